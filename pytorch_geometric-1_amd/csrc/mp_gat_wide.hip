// Node-wise kernels of the GATConv path for heads of any width (C % 4 == 0, a
// head possibly wider than one 256-feature tile, H * C any size): the shapes
// the reference's own GAT stacks use (ConvexPruning.py:209-214: heads = 1,
// out_channels drawn at random by ContractionLayerCoefficients, :106-114).
// The per-head dot products are taken per node here, so the edge passes
// (GatRed non-own forward in mp_gat_fwd.hip, GatBwdWideRed backward below, on
// the engine of mp_agg.h) need no cross-lane reduction per slot.  One wave per
// node; a head is walked in 256-feature chunks (lane = 4 features), each lane
// keeps its running partial across the chunks (separately rounded, chunk
// order), then one 64-lane shuffle-xor tree (group_sum) per head.
#include "mp_agg.h"

namespace mp {

constexpr int kWideWaves = 4;  // waves per block

// sum over a head's features [h*C, h*C + C) of a[.] * (b[.] - sub[.]) for row
// pointers a, b (sub optional: b holds out = agg + bias, sub the bias; lane
// partials in chunk order, then the wave tree); every lane gets the sum
__device__ __forceinline__ float head_dot(const float* __restrict__ a, const float* __restrict__ b, int C,
                                         int lane, const float* __restrict__ sub = nullptr) {
  float t = 0.f;
  for (int c0 = 0; c0 < C; c0 += 256) {
    const int c = c0 + 4 * lane;
    if (c < C) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(a + c);
      f32x4 y = *reinterpret_cast<const f32x4*>(b + c);
      if (sub) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(sub + c);
        y.x = __fsub_rn(y.x, d.x);
        y.y = __fsub_rn(y.y, d.y);
        y.z = __fsub_rn(y.z, d.z);
        y.w = __fsub_rn(y.w, d.w);
      }
      t = __builtin_fmaf(x.x, y.x, t);
      t = __builtin_fmaf(x.y, y.y, t);
      t = __builtin_fmaf(x.z, y.z, t);
      t = __builtin_fmaf(x.w, y.w, t);
    }
  }
  return group_sum(t, 64);
}

// a_dst[n,h] = <xw[n,h,:], att[h, 0:C]>,  a_src[n,h] = <xw[n,h,:], att[h, C:2C]>
__global__ __launch_bounds__(64 * kWideWaves) void k_gat_node_scores_wide(const float* __restrict__ xw,
                                                                         int64_t n_nodes, int32_t H, int32_t C,
                                                                         const float* __restrict__ att,
                                                                         float* __restrict__ a_src,
                                                                         float* __restrict__ a_dst) {
  const int lane = lane_id();
  const int64_t HC = (int64_t)H * C;
  const int64_t nw = (int64_t)gridDim.x * kWideWaves;
  for (int64_t n = (int64_t)blockIdx.x * kWideWaves + (threadIdx.x >> 6); n < n_nodes; n += nw) {
    for (int h = 0; h < H; ++h) {
      const float* row = xw + n * HC + (int64_t)h * C;
      const float* at = att + (int64_t)h * 2 * C;
      const float sd = head_dot(row, at, C, lane);
      const float ss = head_dot(row, at + C, C, lane);
      if (lane == 0) {
        a_dst[n * H + h] = sd;
        a_src[n * H + h] = ss;
      }
    }
  }
}

// Backward prologue after the training forward, per (node n, head h):
//   rs = <g[n,h,:], agg[n,h,:]>,  pack[n,h] = (a_dst, m, 1/den, rs),
//   (bias != nullptr: agg holds out = agg + bias, rs over out - bias)
//   grad_a_dst[n,h] = <g[n,h,:], agg2[n,h,:]> - rs * row_s2[n,h]
__global__ __launch_bounds__(64 * kWideWaves) void k_gat_bwd_prep_wide(
    const float* __restrict__ g, int64_t ldg, const float* __restrict__ agg, int64_t lda,
    const float* __restrict__ bias, const float* __restrict__ agg2, const float* __restrict__ s2,
    const float* __restrict__ a_dst,
    const float* __restrict__ stats, int64_t n, int32_t H, int32_t C, float* __restrict__ pack,
    float* __restrict__ ga_dst) {
  const int lane = lane_id();
  const int64_t HC = (int64_t)H * C;
  const int64_t nw = (int64_t)gridDim.x * kWideWaves;
  for (int64_t r = (int64_t)blockIdx.x * kWideWaves + (threadIdx.x >> 6); r < n; r += nw) {
    for (int h = 0; h < H; ++h) {
      const int64_t o = (int64_t)h * C;
      const float rs = head_dot(g + r * ldg + o, agg + r * lda + o, C, lane, bias ? bias + o : nullptr);
      const float t2 = head_dot(g + r * ldg + o, agg2 + r * HC + o, C, lane);
      if (lane == 0) {
        const int64_t q = r * H + h;
        f32x4 v = {a_dst[q], stats[2 * q], 1.f / stats[2 * q + 1], rs};
        *reinterpret_cast<f32x4*>(pack + 4 * q) = v;
        ga_dst[q] = stats[2 * q + 1] == 1.f ? 0.f : __builtin_fmaf(-rs, s2[q], t2);  // one-hot row: 0
      }
    }
  }
}

// Backward epilogue after GatBwdWideRed, per (node j, head h):
//   ga_src[j,h] = <acc2[j,h,:], xw[j,h,:]> - sc[j,h]      (sc in, ga_src out, in place)
//   gx[j,h,:]  += ga_src[j,h] att[h, C:2C] + ga_dst[j,h] att[h, 0:C]
__global__ __launch_bounds__(64 * kWideWaves) void k_gat_bwd_epilogue_wide(
    float* __restrict__ gx, const float* __restrict__ acc2, const float* __restrict__ xw,
    const float* __restrict__ att, const float* __restrict__ ga_dst, float* __restrict__ sc_ga_src, int64_t n,
    int32_t H, int32_t C) {
  const int lane = lane_id();
  const int64_t HC = (int64_t)H * C;
  const int64_t nw = (int64_t)gridDim.x * kWideWaves;
  for (int64_t j = (int64_t)blockIdx.x * kWideWaves + (threadIdx.x >> 6); j < n; j += nw) {
    for (int h = 0; h < H; ++h) {
      const int64_t o = j * HC + (int64_t)h * C;
      const int64_t q = j * H + h;
      const float gs = head_dot(acc2 + o, xw + o, C, lane) - sc_ga_src[q];
      const float gd = ga_dst[q];
      const float* at = att + (int64_t)h * 2 * C;
      for (int c = 4 * lane; c < C; c += 256) {
        f32x4 v = *reinterpret_cast<f32x4*>(gx + o + c);
        const f32x4 ad = *reinterpret_cast<const f32x4*>(at + c);
        const f32x4 as = *reinterpret_cast<const f32x4*>(at + C + c);
        v.x = __builtin_fmaf(gd, ad.x, __builtin_fmaf(gs, as.x, v.x));
        v.y = __builtin_fmaf(gd, ad.y, __builtin_fmaf(gs, as.y, v.y));
        v.z = __builtin_fmaf(gd, ad.z, __builtin_fmaf(gs, as.z, v.z));
        v.w = __builtin_fmaf(gd, ad.w, __builtin_fmaf(gs, as.w, v.w));
        *reinterpret_cast<f32x4*>(gx + o + c) = v;
      }
      __builtin_amdgcn_wave_barrier();  // every lane has read sc before lane 0 overwrites it
      if (lane == 0) sc_ga_src[q] = gs;
    }
  }
}

static unsigned wide_blocks(int64_t n) {
  int64_t b = (n + kWideWaves - 1) / kWideWaves;
  if (b > 16384) b = 16384;
  return (unsigned)(b < 1 ? 1 : b);
}

static bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }

// GATConv backward for heads of any width (C % 4 == 0; a head may span several
// feature tiles, so no per-slot dot product is possible): over the TRANSPOSED
// CSR (row j = source), with alpha_ij rebuilt from the destination's pack
// (a_dst, m, 1/den, rs) and the row's own a_src[j,h], lk = leaky'(score):
//   acc_j  += alpha d g_i              (message part of d xw_j; d = dropout factor)
//   acc2_j += lk alpha d g_i
//   sc_j   += lk alpha rs_i            (per head)
// The per-edge d score never forms: d a_src_j = sum_i lk alpha (d <g_i, xw_j> - rs_i)
// = <acc2_j, xw_j>_h - sc_j, a node-wise dot product taken after this pass
// (mp_gat_backward_epilogue_wide_f32).  Rows write acc to out, acc2 to out2 and
// sc to ga; every lane of a head holds the same sc.  Elementwise per slot:
// FMA and the hardware exp (gradients are tolerance-checked).
template <int VEC, bool DR = false>
struct GatBwdWideRed : RedFlags {
  static constexpr bool kEid = DR;  // the dropout key: each edge's dst-CSR slot
  static constexpr bool kGatWide = true;
  static constexpr bool kDrop = DR;
  static constexpr bool kStat = true;
  struct Part {
    float v[VEC];
    float v2[VEC];
    float s;
  };
  float acc[VEC], acc2[VEC];
  float sc, as;
  int h;

  __device__ GatBwdWideRed(const AggArgs& p, int f, bool act) : h(act ? f / p.C : 0) {}

  __device__ __forceinline__ void begin(const AggArgs& p, int64_t row, bool, int, bool) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = acc2[k] = 0.f;
    sc = 0.f;
    as = p.a_src[row * p.H + h];
  }
  __device__ __forceinline__ void consume_gatw(const AggArgs& p, const Frag<VEC>& v, f32x4 q,
                                               [[maybe_unused]] uint32_t dbits) {
    const float score = as + q.x;
    const float lk = score > 0.f ? 1.f : p.slope;
    const float alpha = __expf(score * lk - q.y) * q.z;
    // one-hot softmax row (see GatBwdRed::consume_gatb): its d score is 0, so the edge adds
    // nothing to d a_src's two node-wise sums (acc2, sc)
    const bool one_hot = q.z == 1.f && alpha == 1.f;
    sc = one_hot ? sc : __builtin_fmaf(lk * alpha, q.w, sc);
    float aw = alpha;
    if constexpr (DR) aw = alpha * drop_factor(p, dbits, h);
    const float law = one_hot ? 0.f : lk * aw;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      acc[k] = __builtin_fmaf(aw, v.v[k], acc[k]);
      acc2[k] = __builtin_fmaf(law, v.v[k], acc2[k]);
    }
  }
  __device__ __forceinline__ void consume(const Frag<VEC>&, float, int, float) {}
  __device__ __forceinline__ void save(PRef r, bool stat_writer) const {
    Frag<VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
    store_frag<VEC>(r.v, o);
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = acc2[k];
    store_frag<VEC>(r.v2, o);
    if (stat_writer) r.st[0] = sc;
  }
  static __device__ __forceinline__ Part load(PRef r) {
    Frag<VEC> o = load_frag<VEC>(r.v);
    Frag<VEC> o2 = load_frag<VEC>(r.v2);
    Part q;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      q.v[k] = o.v[k];
      q.v2[k] = o2.v[k];
    }
    q.s = r.st[0];
    return q;
  }
  __device__ __forceinline__ void set(const Part& q) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      acc[k] = q.v[k];
      acc2[k] = q.v2[k];
    }
    sc = q.s;
  }
  __device__ __forceinline__ void merge(const Part& q) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      acc[k] += q.v[k];
      acc2[k] += q.v2[k];
    }
    sc += q.s;
  }
  __device__ __forceinline__ Part part() const {
    Part q;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      q.v[k] = acc[k];
      q.v2[k] = acc2[k];
    }
    q.s = sc;
    return q;
  }
  __device__ __forceinline__ void finish(const AggArgs& p, int64_t row, int64_t, int f, bool act, bool with_bias = true) {
    if (!act) return;
    Frag<VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
    store_out<VEC>(p.out + row * p.ldo + f, o);
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = acc2[k];
    store_out<VEC>(p.out2 + row * (int64_t)p.F + f, o);
    if (f % p.C == 0) p.ga[row * p.H + h] = sc;
  }
};

}  // namespace mp

using namespace mp;

extern "C" {

int mp_gat_wide_ok(int32_t H, int32_t C) { return H > 0 && C > 0 && C % 4 == 0 ? 1 : 0; }

int mp_gat_node_scores_wide_f32(const float* xw, int64_t n_nodes, int32_t H, int32_t C, const float* att,
                                float* a_src, float* a_dst, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(mp_gat_wide_ok(H, C) && n_nodes >= 0, "mp_gat_node_scores_wide_f32: needs C %% 4 == 0");
  if (n_nodes == 0) return MP_OK;
  MP_CHECK_ARG(xw && att && a_src && a_dst, "mp_gat_node_scores_wide_f32: null pointer");
  MP_CHECK_ARG(al16(xw) && al16(att), "mp_gat_node_scores_wide_f32: xw and att must be 16-byte aligned");
  k_gat_node_scores_wide<<<wide_blocks(n_nodes), 64 * kWideWaves, 0, as_stream(stream)>>>(xw, n_nodes, H, C, att,
                                                                                          a_src, a_dst);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

int mp_gat_backward_prep_wide_f32(const float* grad_out, int64_t ldg, const float* agg, int64_t lda,
                                  const float* bias, const float* agg2, const float* row_s2, const float* a_dst, const float* row_stats,
                                  int64_t n, int32_t H, int32_t C, float* pack, size_t pack_bytes,
                                  float* grad_a_dst, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(mp_gat_wide_ok(H, C) && n >= 0, "mp_gat_backward_prep_wide_f32: needs C %% 4 == 0");
  if (n == 0) return MP_OK;
  MP_CHECK_ARG(grad_out && agg && agg2 && row_s2 && a_dst && row_stats && pack && grad_a_dst,
               "mp_gat_backward_prep_wide_f32: null pointer");
  MP_CHECK_EXTENT("mp_gat_backward_prep_wide_f32", "pack", pack_bytes, (size_t)n * H * 16);
  const int64_t F = (int64_t)H * C;
  MP_CHECK_ARG(ldg >= F && lda >= F && ldg % 4 == 0 && lda % 4 == 0, "mp_gat_backward_prep_wide_f32: bad ld");
  MP_CHECK_ARG(al16(grad_out) && al16(agg) && al16(agg2) && al16(pack) && al16(bias),
               "mp_gat_backward_prep_wide_f32: 16-byte alignment required");
  k_gat_bwd_prep_wide<<<wide_blocks(n), 64 * kWideWaves, 0, as_stream(stream)>>>(
      grad_out, ldg, agg, lda, bias, agg2, row_s2, a_dst, row_stats, n, H, C, pack, grad_a_dst);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

int mp_gat_backward_epilogue_wide_f32(float* grad_xw, const float* acc2, const float* xw, const float* att,
                                      const float* grad_a_dst, float* sc_grad_a_src, int64_t n, int32_t H,
                                      int32_t C, void* stream) {
  MP_DEVICE_GUARD(stream);
  MP_CHECK_ARG(mp_gat_wide_ok(H, C) && n >= 0, "mp_gat_backward_epilogue_wide_f32: needs C %% 4 == 0");
  if (n == 0) return MP_OK;
  MP_CHECK_ARG(grad_xw && acc2 && xw && att && grad_a_dst && sc_grad_a_src,
               "mp_gat_backward_epilogue_wide_f32: null pointer");
  MP_CHECK_ARG(al16(grad_xw) && al16(acc2) && al16(xw) && al16(att),
               "mp_gat_backward_epilogue_wide_f32: 16-byte alignment required");
  k_gat_bwd_epilogue_wide<<<wide_blocks(n), 64 * kWideWaves, 0, as_stream(stream)>>>(
      grad_xw, acc2, xw, att, grad_a_dst, sc_grad_a_src, n, H, C);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

int mp_gat_backward_wide_f32(const mp_csr* gt, const float* grad_out, int64_t ldg, const float* a_src,
                             const float* pack, int32_t H, int32_t C, float slope, uint64_t seed, float p_drop,
                             const int32_t* drop_ids, float* grad_xw, float* acc2, size_t acc2_bytes, float* sc, size_t sc_bytes, void* slab,
                             size_t slab_bytes, int32_t stages, void* stream) {
  MP_DEVICE_GUARD(stream);
  int rc = check_graph(gt, "mp_gat_backward_wide_f32");
  if (rc) return rc;
  MP_CHECK_ARG(H > 0 && C > 0 && C % 4 == 0, "mp_gat_backward_wide_f32: needs C %% 4 == 0");
  if (p_drop > 0.f) {
    rc = drop_check(p_drop, H, "mp_gat_backward_wide_f32");
    if (rc) return rc;
  }
  MP_CHECK_ARG(grad_out && a_src && pack && grad_xw && acc2 && sc, "mp_gat_backward_wide_f32: null pointer");
  const int F = H * C;
  MP_CHECK_ARG(ldg >= F && ldg % 4 == 0, "mp_gat_backward_wide_f32: ldg < H*C or not a multiple of 4");
  MP_CHECK_ARG((uintptr_t)grad_out % 16 == 0 && (uintptr_t)grad_xw % 16 == 0 && (uintptr_t)acc2 % 16 == 0 &&
                   (uintptr_t)pack % 16 == 0,
               "mp_gat_backward_wide_f32: grad_out, grad_xw, acc2, pack must be 16-byte aligned");
  MP_CHECK_ARG(slab && slab_bytes >= mp_gat_train_slab_bytes(gt, H, C),
               "mp_gat_backward_wide_f32: slab workspace too small (mp_gat_train_slab_bytes)");
  MP_CHECK_EXTENT("mp_gat_backward_wide_f32", "acc2", acc2_bytes, (size_t)gt->n_rows * F * 4);
  MP_CHECK_EXTENT("mp_gat_backward_wide_f32", "sc", sc_bytes, (size_t)gt->n_rows * H * 4);
  AggArgs a{};
  fill_graph(a, gt);
  a.F = F;
  a.x = grad_out;
  a.ldx = ldg;
  a.out = grad_xw;
  a.ldo = F;
  a.out2 = acc2;
  a.ga = sc;
  a.a_src = a_src;
  a.pack = reinterpret_cast<const f32x4*>(pack);
  a.H = H;
  a.C = C;
  a.slope = slope;
  carve_slabs(a, slab, kSlabStat | kSlabV2);
  hipStream_t s = as_stream(stream);
  const int lanes = F >= 256 ? 64 : (F / 4 <= 4 ? 4 : next_pow2(F / 4));
  if (p_drop > 0.f) {
    set_drop(a, seed, p_drop, drop_ids);
    return launch<GatBwdWideRed<4, true>, 4>(a, stages, s, lanes);
  }
  return launch<GatBwdWideRed<4>, 4>(a, stages, s, lanes);
}

}  // extern "C"
