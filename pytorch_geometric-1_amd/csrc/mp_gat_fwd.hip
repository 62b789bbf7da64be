// The fused GATConv forward on the merge-path engine (mp_agg.h) for gfx950:
// one pass with an online softmax per (row, head) -- inference
// (mp_gat_aggregate*_f32, mp_gat_forward_f32) and training, which also leaves
// what makes the backward's d a_dst node-wise (mp_gat_*_train*_f32), with
// attention dropout; and the dropout keep mask itself (mp_gat_dropout_keep).
#include "mp_agg.h"

namespace mp {

#ifndef MP_U_GAT_TRAIN
#define MP_U_GAT_TRAIN 4
#endif
constexpr int kU_GatTrain = MP_U_GAT_TRAIN;  // x-row loads in flight per task of the GAT training forward
                                             // (A/B U=4/6/8: 8.36/8.57/8.52 ms)

// GATConv [U6] + utils.softmax [U3], online: per (row, head) running max m,
// denominator s and accumulator acc, rescaled when the max grows.  Every lane
// of a head carries the same m/s (no cross-lane traffic).
//
// OWN: a_src[j, h] is recomputed from the gathered row itself,
//   a_src[j,h] = <xw[j,h,:], att[h,C:2C]>  (lane partial of its VEC features,
// then group_sum over the head's lanes -- the same arithmetic, in the same
// order, as k_gat_node_scores_wave, so bitwise the value that kernel stores).
// It saves the per-slot a_src gather (one 256-B L1-queue segment per slot on
// top of the row's four).
//
// TR (training forward): also accumulates, with the same online rescaling,
//   acc2 = sum_k alpha_k leaky'_k x_k  and  s2 = sum_k alpha_k leaky'_k
// (leaky' = 1 or slope at the pre-activation a_src + a_dst), written to
// out2 / row_s2.  They make the backward's d a_dst node-wise:
//   d a_dst[i,h] = sum_j de_ij = <g_i, acc2_i>_h - rs_i s2_i
// (de_ij = alpha_ij (<g_i, xw_j> - rs_i) leaky'_ij), so the backward writes no
// per-edge d score and needs no segmented pass over it.
//
// ND (node scores, needs OWN): a_dst[i, h] and a_src[i, h] of each destination
// row come from the row's own xw, loaded at begin() and reduced at the first
// slot (its load completes before the first gathered row's, so the wait is
// hidden) with the node-score kernel's arithmetic -- bitwise its values; the
// row's owner task writes both to a_src_out / a_dst_out, so no separate
// node-score pass over xw is needed.
// DR (attention dropout, training): slot weight pe * keep / (1 - p) on the
// aggregates (acc, acc2), the softmax sums (s, s2) unchanged.
template <int VEC, bool OWN = false, bool TR = false, bool ND = false, bool DR = false>
struct GatRed : RedFlags {
  static_assert(!ND || OWN, "in-kernel node scores reuse the own-a_src reduction");
  static constexpr bool kGat = true;
  static constexpr bool kOwnAs = OWN;
  static constexpr bool kNodeScores = ND;
  static constexpr bool kDrop = DR;
  static constexpr bool kStat = true;
  static constexpr bool kTrain = TR;
  static constexpr int kUTrain = kU_GatTrain;
  struct Part {
    float v[VEC];
    float m, s;
    float v2[TR ? VEC : 1];
    float s2;
  };
  float acc[VEC];
  float m, s, ad;
  [[maybe_unused]] float acc2[TR ? VEC : 1];
  [[maybe_unused]] float s2 = 0.f;
  int h;
  [[maybe_unused]] float y[OWN ? VEC : 1];
  [[maybe_unused]] int hl = 1;
  [[maybe_unused]] Frag<ND ? VEC : 1> rowv;  // the destination row's own xw (ND)
  [[maybe_unused]] bool need_ad = false, own_row = false, lead = false;
  [[maybe_unused]] int c_ = 0;               // this lane's first feature within its head (ND)
  [[maybe_unused]] int64_t row_ = 0;

  __device__ GatRed(const AggArgs& p, int f, bool act) : h(act ? f / p.C : 0) {
    if constexpr (OWN) {
      hl = p.C / VEC;
      const int c = act ? f % p.C : 0;
      Frag<VEC> o = load_frag<VEC>(p.att + (int64_t)h * 2 * p.C + p.C + c);
#pragma unroll
      for (int k = 0; k < VEC; ++k) y[k] = act ? o.v[k] : 0.f;
      if constexpr (ND) {
        c_ = c;
        lead = act && c == 0;
      }
    }
  }
  // the row's scores from rowv; the owner writes them (every lane of the
  // wave runs this together: the group sums are cross-lane)
  __device__ __forceinline__ void node_scores(const AggArgs& p) {
    if constexpr (ND) {
      // att_dst slice: an L1-resident 16-B load per row rather than 4 VGPRs held
      // through the slot loop (keeps the kernel at the OWN path's occupancy)
      const Frag<VEC> yd = load_frag<VEC>(p.att + (int64_t)h * 2 * p.C + c_);
      float t = rowv.v[0] * yd.v[0];
#pragma unroll
      for (int k = 1; k < VEC; ++k) t = t + rowv.v[k] * yd.v[k];
      ad = group_sum(t, hl);
      const float as_own = own_as(rowv);
      need_ad = false;
      if (own_row && lead) {
        p.a_dst_out[row_ * p.H + h] = ad;
        p.a_src_out[row_ * p.H + h] = as_own;
      }
    }
  }
  // before a partial of an owned row is saved (its task may have seen none of
  // its slots): make sure the row's scores were written
  __device__ __forceinline__ void flush_scores(const AggArgs& p) {
    if constexpr (ND) {
      if (need_ad) node_scores(p);
    }
  }
  // <row, att_src> over the head's lanes: v.x*y.x + v.y*y.y + ... separately
  // rounded left to right (-ffp-contract=off), then group_sum
  __device__ __forceinline__ float own_as(const Frag<VEC>& v) const {
    float t = v.v[0] * y[0];
#pragma unroll
    for (int k = 1; k < VEC; ++k) t = t + v.v[k] * y[k];
    return group_sum(t, hl);
  }

  __device__ __forceinline__ void begin(const AggArgs& p, int64_t row, bool owned, int f, bool act) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    if constexpr (TR) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc2[k] = 0.f;
      s2 = 0.f;
    }
    m = -INFINITY;
    s = 0.f;
    if constexpr (ND) {
      rowv = load_frag<VEC>(p.x + row * p.ldx + (act ? f : 0));
      need_ad = true;
      own_row = owned;
      row_ = row;
    } else {
      ad = p.a_dst[row * p.H + h];
    }
  }
  __device__ __forceinline__ void consume_gat(const AggArgs& p, const Frag<VEC>& v, float as,
                                              [[maybe_unused]] uint32_t dbits = 0) {
    float a = as + ad;
    [[maybe_unused]] const bool pos = a > 0.f;  // leaky' = 1 : slope (the backward's test)
    a = a > 0.f ? a : a * p.slope;  // F.leaky_relu
    // mn = fmaxf(m, a); sc = expf(m - mn); pe = expf(a - mn) with one exp:
    // one of the two arguments is x - x, i.e. 0 (exp 1) or NaN for an
    // infinite x, so (x - x) + 1 reproduces it bit for bit, NaNs included
    // (config 3: 7.81 -> 7.74 ms)
    const bool up = a > m;
    const float e = expf(up ? m - a : a - m);
    const float sc = up ? e : (m - m) + 1.f;
    const float pe = up ? (a - a) + 1.f : e;
    s = s * sc + pe;
    [[maybe_unused]] float dsc = 1.f;
    if constexpr (DR) {
      dsc = drop_factor(p, dbits, h);
      const float pd = pe * dsc;
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = acc[k] * sc + pd * v.v[k];
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] = acc[k] * sc + pe * v.v[k];
    }
    if constexpr (TR) {
      const float pl = pos ? pe : pe * p.slope;
      s2 = s2 * sc + pl;
      const float pld = DR ? pl * dsc : pl;
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc2[k] = acc2[k] * sc + pld * v.v[k];
    }
    m = up ? a : m;
  }
  __device__ __forceinline__ void consume(const Frag<VEC>&, float, int, float) {}
  __device__ __forceinline__ void save(PRef r, bool stat_writer) const {
    Frag<VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
    store_frag<VEC>(r.v, o);
    if (stat_writer) {
      r.st[0] = m;
      r.st[1] = s;
    }
    if constexpr (TR) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) o.v[k] = acc2[k];
      store_frag<VEC>(r.v2, o);
      if (stat_writer) *r.s2 = s2;
    }
  }
  static __device__ __forceinline__ Part load(PRef r) {
    Frag<VEC> o = load_frag<VEC>(r.v);
    Part q;
#pragma unroll
    for (int k = 0; k < VEC; ++k) q.v[k] = o.v[k];
    q.m = r.st[0];
    q.s = r.st[1];
    if constexpr (TR) {
      Frag<VEC> o2 = load_frag<VEC>(r.v2);
#pragma unroll
      for (int k = 0; k < VEC; ++k) q.v2[k] = o2.v[k];
      q.s2 = *r.s2;
    }
    return q;
  }
  __device__ __forceinline__ void set(const Part& q) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = q.v[k];
    m = q.m;
    s = q.s;
    if constexpr (TR) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc2[k] = q.v2[k];
      s2 = q.s2;
    }
  }
  __device__ __forceinline__ void merge(const Part& q) {
    float mn = fmaxf(m, q.m);
    float c0 = expf(m - mn), c1 = expf(q.m - mn);
    s = s * c0 + q.s * c1;
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = acc[k] * c0 + q.v[k] * c1;
    if constexpr (TR) {
      s2 = s2 * c0 + q.s2 * c1;
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc2[k] = acc2[k] * c0 + q.v2[k] * c1;
    }
    m = mn;
  }
  __device__ __forceinline__ Part part() const {
    Part q;
#pragma unroll
    for (int k = 0; k < VEC; ++k) q.v[k] = acc[k];
    q.m = m;
    q.s = s;
    if constexpr (TR) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) q.v2[k] = acc2[k];
      q.s2 = s2;
    }
    return q;
  }
  __device__ __forceinline__ void finish(const AggArgs& p, int64_t row, int64_t, int f, bool act, bool with_bias = true) {
    if constexpr (ND) {
      if (need_ad) node_scores(p);  // a row without slots (the fix-up never begins a row: need_ad false)
    }
    if (!act) return;
    Frag<VEC> o;
    float den = s + 1e-16f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = acc[k] / den;
    if constexpr (TR) {  // the pre-bias aggregate the backward's rs needs
      if (p.agg_nb) store_out<VEC>(p.agg_nb + row * (int64_t)p.F + f, o);
    }
    if (p.bias) {
      Frag<VEC> b = load_frag<VEC>(p.bias + f);
#pragma unroll
      for (int k = 0; k < VEC; ++k) o.v[k] = o.v[k] + b.v[k];
    }
    store_out<VEC>(p.out + row * p.ldo + f, o);
    if (p.row_stats && (f % p.C == 0)) {
      p.row_stats[(row * p.H + h) * 2] = m;
      p.row_stats[(row * p.H + h) * 2 + 1] = den;
    }
    if constexpr (TR) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) o.v[k] = acc2[k] / den;
      store_out<VEC>(p.out2 + row * (int64_t)p.F + f, o);
      if (f % p.C == 0) p.row_s2[row * p.H + h] = s2 / den;
    }
  }
};

// the dropout keep bits of slots [0, n) (mp_gat_dropout_keep: tests, host-side masks)
__global__ void k_gat_dropout_keep(AggArgs p, int64_t n, uint32_t* bits) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) bits[i] = drop_bits(p, p.drop_ids ? (int64_t)p.drop_ids[i] : i);
}

}  // namespace mp

using namespace mp;

extern "C" {

size_t mp_gat_slab_bytes(const mp_csr* g, int32_t H, int32_t C) {
  if (!g || H <= 0 || C <= 0) return 256;
  return slab_layout(g->n_waves, H * C, H, kSlabStat).total;
}

size_t mp_gat_train_slab_bytes(const mp_csr* g, int32_t H, int32_t C) {
  if (!g || H <= 0 || C <= 0) return 256;
  return slab_layout(g->n_waves, H * C, H, kSlabStat | kSlabV2 | kSlabS2).total;
}

int mp_gat_train_ok(int32_t H, int32_t C) {
  const int hl4 = C / 4;
  return H > 0 && C > 0 && C % 4 == 0 && hl4 <= 64 && (hl4 & (hl4 - 1)) == 0 ? 1 : 0;
}

int mp_gat_aggregate_f32(const mp_csr* g, const float* xw, const float* a_src, const float* a_dst,
                         int32_t H, int32_t C, float slope, const float* bias, float* out,
                         int64_t ldo, float* row_stats, void* slab, size_t slab_bytes,
                         int32_t stages, void* stream) {
  return mp_gat_aggregate_att_f32(g, xw, a_src, a_dst, nullptr, H, C, slope, bias, out, ldo, row_stats, slab,
                                  slab_bytes, stages, stream);
}

int mp_gat_aggregate_att_f32(const mp_csr* g, const float* xw, const float* a_src, const float* a_dst,
                             const float* att, int32_t H, int32_t C, float slope, const float* bias, float* out,
                             int64_t ldo, float* row_stats, void* slab, size_t slab_bytes, int32_t stages,
                             void* stream) {
  MP_DEVICE_GUARD(stream);
  int rc = check_graph(g, "mp_gat_aggregate_f32");
  if (rc) return rc;
  MP_CHECK_ARG(H > 0 && C > 0, "mp_gat_aggregate_f32: H, C must be positive");
  MP_CHECK_ARG(xw && a_src && a_dst && out, "mp_gat_aggregate_f32: null input");
  const int F = H * C;
  MP_CHECK_ARG(ldo >= F, "mp_gat_aggregate_f32: ldo < H*C");
  MP_CHECK_ARG(slab != nullptr && slab_bytes >= mp_gat_slab_bytes(g, H, C),
               "mp_gat_aggregate_f32: slab workspace too small");
  AggArgs a{};
  fill_graph(a, g);
  a.F = F;
  a.x = xw;
  a.ldx = F;
  a.out = out;
  a.ldo = ldo;
  a.bias = bias;
  a.a_src = a_src;
  a.a_dst = a_dst;
  a.H = H;
  a.C = C;
  a.slope = slope;
  a.row_stats = row_stats;
  carve_slabs(a, slab, kSlabStat);
  hipStream_t s = as_stream(stream);
  int vec = pick_shape(F, F, xw, ldo, out).vec;
  if (vec == 2 && F <= 64) vec = 1;
  while (vec > 1 && C % vec != 0) vec >>= 1;  // a lane's features must share a head
  // a_src from the gathered rows: the node-score kernel's 4-feature lane
  // partials and head groups of C/4 lanes (a power of two <= 64)
  const int hl4 = C / 4;
  if (att && vec == 4 && C % 4 == 0 && hl4 <= 64 && (hl4 & (hl4 - 1)) == 0 && (uintptr_t)att % 16 == 0) {
    a.att = att;
    return launch<GatRed<4, true>, 4>(a, stages, s, F >= 256 ? kGatLanes : 64);
  }
  switch (vec) {
    case 4: return launch<GatRed<4>, 4>(a, stages, s, F >= 256 ? kGatLanes : 64);
    case 2: return launch<GatRed<2>, 2>(a, stages, s);
    default: return launch<GatRed<1>, 1>(a, stages, s);
  }
}

int mp_gat_forward_f32(const mp_csr* g, const float* xw, const float* att, int32_t H, int32_t C, float slope,
                       const float* bias, float* out, int64_t ldo, float* a_src, float* a_dst, float* row_stats,
                       void* slab, size_t slab_bytes, int32_t stages, void* stream) {
  MP_DEVICE_GUARD(stream);
  int rc = check_graph(g, "mp_gat_forward_f32");
  if (rc) return rc;
  MP_CHECK_ARG(mp_gat_train_ok(H, C), "mp_gat_forward_f32: needs C %% 4 == 0 and C/4 a power of two <= 64");
  MP_CHECK_ARG(xw && att && out && a_src && a_dst, "mp_gat_forward_f32: null pointer");
  MP_CHECK_ARG(g->n_cols == g->n_rows, "mp_gat_forward_f32: the graph must be square (row i's own xw is row i)");
  const int F = H * C;
  MP_CHECK_ARG(ldo >= F && ldo % 4 == 0, "mp_gat_forward_f32: ldo < H*C or not a multiple of 4");
  MP_CHECK_ARG((uintptr_t)xw % 16 == 0 && (uintptr_t)att % 16 == 0 && (uintptr_t)out % 16 == 0 &&
                   (uintptr_t)bias % 16 == 0,
               "mp_gat_forward_f32: xw, att, bias, out must be 16-byte aligned");
  MP_CHECK_ARG(slab != nullptr && slab_bytes >= mp_gat_slab_bytes(g, H, C),
               "mp_gat_forward_f32: slab workspace too small");
  AggArgs a{};
  fill_graph(a, g);
  a.F = F;
  a.x = xw;
  a.ldx = F;
  a.out = out;
  a.ldo = ldo;
  a.bias = bias;
  a.a_src_out = a_src;
  a.a_dst_out = a_dst;
  a.att = att;
  a.H = H;
  a.C = C;
  a.slope = slope;
  a.row_stats = row_stats;
  carve_slabs(a, slab, kSlabStat);
  return launch<GatRed<4, true, false, true>, 4>(a, stages, as_stream(stream), F >= 256 ? kGatLanes : 64);
}

static int gat_train(const mp_csr* g, const float* xw, const float* a_src, const float* a_dst, const float* att,
                     int32_t H, int32_t C, float slope, const float* bias, float* out, int64_t ldo, float* agg,
                     float* row_stats, float* out2, float* row_s2, void* slab, size_t slab_bytes, int32_t stages,
                     void* stream, float* as_out, float* ad_out, uint64_t drop_seed = 0, float p_drop = 0.f,
                     const int32_t* drop_ids = nullptr) {
  MP_DEVICE_GUARD(stream);
  int rc = check_graph(g, "mp_gat_aggregate_train_f32");
  if (rc) return rc;
  // a_src from each gathered row (OWN) when a head fits one lane group (C/4 a
  // power of two <= 64); any other C % 4 == 0 reads the node-score arrays
  const bool own = mp_gat_train_ok(H, C) && att != nullptr;
  MP_CHECK_ARG(H > 0 && C > 0 && C % 4 == 0, "mp_gat_aggregate_train_f32: needs C %% 4 == 0");
  MP_CHECK_ARG(own || (!as_out && a_src && a_dst),
               "mp_gat_aggregate_train_f32: heads with C/4 not a power of two <= 64 need a_src / a_dst inputs");
  MP_CHECK_ARG(xw && out && row_stats && out2 && row_s2, "mp_gat_aggregate_train_f32: null input");
  const int F = H * C;
  MP_CHECK_ARG(ldo >= F, "mp_gat_aggregate_train_f32: ldo < H*C");
  MP_CHECK_ARG((uintptr_t)xw % 16 == 0 && (uintptr_t)att % 16 == 0 && (uintptr_t)out % 16 == 0 && ldo % 4 == 0 &&
                   (uintptr_t)out2 % 16 == 0 && (uintptr_t)agg % 16 == 0 && (uintptr_t)bias % 16 == 0,
               "mp_gat_aggregate_train_f32: xw, att, bias, out, agg, out2 must be 16-byte aligned (ldo %% 4 == 0)");
  MP_CHECK_ARG(slab != nullptr && slab_bytes >= mp_gat_train_slab_bytes(g, H, C),
               "mp_gat_aggregate_train_f32: slab workspace too small");
  AggArgs a{};
  fill_graph(a, g);
  a.F = F;
  a.x = xw;
  a.ldx = F;
  a.out = out;
  a.ldo = ldo;
  a.a_src = a_src;
  a.a_dst = a_dst;
  a.att = att;
  a.H = H;
  a.C = C;
  a.slope = slope;
  a.row_stats = row_stats;
  a.out2 = out2;
  a.row_s2 = row_s2;
  a.bias = bias;
  a.agg_nb = agg;
  a.a_src_out = as_out;  // mp_gat_forward_train_f32: node scores in-kernel
  a.a_dst_out = ad_out;
  carve_slabs(a, slab, kSlabStat | kSlabV2 | kSlabS2);
  const int lanes = F >= 256 ? kGatLanes : 64;
  if (!own) {
    a.att = nullptr;
    if (p_drop > 0.f) {
      set_drop(a, drop_seed, p_drop, drop_ids);
      return launch<GatRed<4, false, true, false, true>, 4>(a, stages, as_stream(stream), lanes);
    }
    return launch<GatRed<4, false, true>, 4>(a, stages, as_stream(stream), lanes);
  }
  if (p_drop > 0.f) {
    set_drop(a, drop_seed, p_drop, drop_ids);
    return launch<GatRed<4, true, true, false, true>, 4>(a, stages, as_stream(stream), lanes);
  }
  if (a.a_src_out) return launch<GatRed<4, true, true, true>, 4>(a, stages, as_stream(stream), lanes);
  return launch<GatRed<4, true, true>, 4>(a, stages, as_stream(stream), F >= 256 ? kGatLanes : 64);
}

int mp_gat_aggregate_train_f32(const mp_csr* g, const float* xw, const float* a_src, const float* a_dst,
                               const float* att, int32_t H, int32_t C, float slope, const float* bias, float* out,
                               int64_t ldo, float* agg, float* row_stats, float* out2, float* row_s2, void* slab,
                               size_t slab_bytes, int32_t stages, void* stream) {
  MP_CHECK_ARG(a_src && a_dst, "mp_gat_aggregate_train_f32: null input");
  return gat_train(g, xw, a_src, a_dst, att, H, C, slope, bias, out, ldo, agg, row_stats, out2, row_s2, slab,
                   slab_bytes, stages, stream, nullptr, nullptr);
}

int mp_gat_forward_train_f32(const mp_csr* g, const float* xw, const float* att, int32_t H, int32_t C, float slope,
                             const float* bias, float* out, int64_t ldo, float* agg, float* row_stats, float* out2,
                             float* row_s2, float* a_src, float* a_dst, void* slab, size_t slab_bytes,
                             int32_t stages, void* stream) {
  MP_CHECK_ARG(a_src && a_dst, "mp_gat_forward_train_f32: null a_src / a_dst");
  MP_CHECK_ARG(!g || g->n_cols == g->n_rows, "mp_gat_forward_train_f32: the graph must be square");
  return gat_train(g, xw, a_src, a_dst, att, H, C, slope, bias, out, ldo, agg, row_stats, out2, row_s2, slab,
                   slab_bytes, stages, stream, a_src, a_dst);
}

int mp_gat_aggregate_train_drop_f32(const mp_csr* g, const float* xw, const float* a_src, const float* a_dst,
                                    const float* att, int32_t H, int32_t C, float slope, const float* bias,
                                    float* out, int64_t ldo, float* agg, float* row_stats, float* out2,
                                    float* row_s2, uint64_t seed, float p_drop, const int32_t* drop_ids, void* slab,
                                    size_t slab_bytes, int32_t stages, void* stream) {
  int rc = drop_check(p_drop, H, "mp_gat_aggregate_train_drop_f32");
  if (rc) return rc;
  MP_CHECK_ARG(a_src && a_dst, "mp_gat_aggregate_train_drop_f32: null input");
  return gat_train(g, xw, a_src, a_dst, att, H, C, slope, bias, out, ldo, agg, row_stats, out2, row_s2, slab,
                   slab_bytes, stages, stream, nullptr, nullptr, seed, p_drop, drop_ids);
}

int mp_gat_dropout_keep(uint64_t seed, float p_drop, int32_t H, int64_t n_slots, const int32_t* drop_ids,
                        uint32_t* bits, void* stream) {
  MP_DEVICE_GUARD(stream);
  int rc = drop_check(p_drop, H, "mp_gat_dropout_keep");
  if (rc) return rc;
  MP_CHECK_ARG(n_slots >= 0, "mp_gat_dropout_keep: negative n_slots");
  if (n_slots == 0) return MP_OK;
  MP_CHECK_ARG(bits != nullptr, "mp_gat_dropout_keep: null bits");
  AggArgs a{};
  a.H = H;
  set_drop(a, seed, p_drop, drop_ids);
  hipLaunchKernelGGL(k_gat_dropout_keep, dim3((unsigned)ceil_div(n_slots, 256)), dim3(256), 0, as_stream(stream), a,
                     n_slots, bits);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

}  // extern "C"

