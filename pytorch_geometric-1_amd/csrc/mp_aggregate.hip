// The plain aggregation on the merge-path engine (mp_agg.h) for gfx950:
// sum / mean / max / min (mp_aggregate_f32, mp_aggregate_tiles_f32), per-head
// weighted sums (mp_aggregate_heads_f32) and the two-pass GAT
// (mp_gat_softmax_aggregate_f32).  Besides the engine's k_agg_main it has two
// main-stage kernels of its own, k_agg_lane (narrow rows, one task per lane)
// and k_agg_flat (slot batches across row boundaries), and the mp_tune table.
// choose() picks between the three: a pure host function of a call's arguments
// and the table that returns the launch as a value (AggLaunch, mp_agg.h) and
// launches nothing; the entry points are check, fill, choose, run, and
// mp_aggregate_kernel_name is the same choice with its main kernel named.
//   * sum uses separately-rounded mul and add (no FMA contraction) in original
//     edge order, i.e. exactly the arithmetic of the reference's materialised
//     `norm*x_j` followed by CPU scatter_add_: rows that fit in one task are
//     bit-identical to the oracle.
#include <atomic>
#include <cxxabi.h>
#include <stdlib.h>
#include <float.h>

#include "mp_agg.h"
#include "mp_flat_ring.h"

// Kernel-shape constants of the plain aggregation (chosen like mp_agg.h's).
namespace mp {
#ifndef MP_U_VEC1_FAR
#define MP_U_VEC1_FAR 8
#endif
constexpr int kU_Vec1Far = MP_U_VEC1_FAR;  // x-row loads in flight per task (VEC=1): scalar-batch sum/mean over an x larger than the Infinity Cache
constexpr int kLaneMaxF = 8;    // rows of 2..this many features: one task per lane (A/B: wins at F=4,8)
constexpr int64_t kSeqTilesMin = 384ll << 20;  // mp_aggregate_tiles_f32: sequential feature tiles above this x
constexpr int kULane = 8;       // slots in flight per lane task

template <int VEC, bool HAS_W, bool MEAN>
struct SumRed : RedFlags {
  static constexpr bool kW = HAS_W;
  struct Part {
    float v[VEC];
  };
  float acc[VEC];
  // the bias features of this lane, read once per task (preload_bias) by the
  // short-row passes of mp_aggregate_tiles_f32 (k_agg_flat XM != 0) and by the
  // rolling gather window of k_agg_flat's scalar-batch loop
  float bv[VEC];
  bool pre = false;
  int h = 0;  // unused (GAT only)

  __device__ SumRed() {}
  __device__ SumRed(const AggArgs&, int, bool) {}

  // A bias load per row is waited for at the row's end, and the wait (vmcnt
  // retires in order) also drains every gather issued before it -- the next
  // rows' prefetched batch.  On the sharded step's short rows (4.4 edges a row)
  // that cost the interior pass 19 % (tools/exp_interior.py: 0.287 -> 0.245
  // ms), so the tile launches take it once per task.  On the one-GPU kernel's
  // long rows the per-row load measured 1-3 % faster while the loop drained its
  // gathers at every batch's end anyway; under the rolling gather window it is
  // the slower form (config 2, ring of 4: 6.79 ms against 6.45 ms with the bias
  // per task), so the window's instances take it once per task too.  Whole-batch
  // instances outside the tile launches keep the load per row.
  __device__ __forceinline__ void preload_bias(const AggArgs& p, int f, bool act) {
    if (p.bias && act) {
      Frag<VEC> b = load_frag<VEC>(p.bias + f);
#pragma unroll
      for (int k = 0; k < VEC; ++k) bv[k] = b.v[k];
    }
    pre = true;
  }
  __device__ __forceinline__ Frag<VEC> bias_of(const AggArgs& p, int f) const {
    if (pre) {
      Frag<VEC> b;
#pragma unroll
      for (int k = 0; k < VEC; ++k) b.v[k] = bv[k];
      return b;
    }
    return load_frag<VEC>(p.bias + f);
  }

  // SETTLE: wait for the row's initial value where it is loaded.  Left pending,
  // the load is one that every later accumulate may have to wait for, on every
  // path that reaches it: the compiler then puts s_waitcnt vmcnt(0) in front of
  // each accumulate of k_agg_flat's scalar-batch loop, and the wave sits until
  // all its gathers have landed before it consumes the first.
  template <bool SETTLE>
  __device__ __forceinline__ void begin_at(const AggArgs& p, int64_t row, bool owned, int f, bool act) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    if (owned && (p.flags & MP_FLAG_INIT_FROM_OUT) && act) {
      Frag<VEC> o = load_frag<VEC>(p.out + row * p.ldo + f);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if constexpr (SETTLE) asm volatile("" : "+v"(o.v[k]));
        acc[k] = o.v[k];
      }
    }
  }
  __device__ __forceinline__ void begin(const AggArgs& p, int64_t row, bool owned, int f, bool act) {
    begin_at<false>(p, row, owned, f, act);
  }
  __device__ __forceinline__ void consume(const Frag<VEC>& v, float wt, int, float) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = __fadd_rn(acc[k], HAS_W ? __fmul_rn(wt, v.v[k]) : v.v[k]);
  }
  // The accumulate so far stays in front of what follows.  k_agg_flat's rolling
  // window refills a ring entry right behind the accumulate that consumed it;
  // with the accumulate moved below the refill, the refill lands in another
  // register and is copied into the entry behind an s_waitcnt vmcnt(0).
  __device__ __forceinline__ void pin() {
#pragma unroll
    for (int k = 0; k < VEC; ++k) asm volatile("" : "+v"(acc[k]) : : "memory");
  }
  __device__ __forceinline__ void save(PRef r, bool) const {
    Frag<VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
    store_frag<VEC>(r.v, o);
  }
  static __device__ __forceinline__ Part load(PRef r) {
    Frag<VEC> o = load_frag<VEC>(r.v);
    Part q;
#pragma unroll
    for (int k = 0; k < VEC; ++k) q.v[k] = o.v[k];
    return q;
  }
  __device__ __forceinline__ void set(const Part& q) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = q.v[k];
  }
  __device__ __forceinline__ void merge(const Part& q) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = __fadd_rn(acc[k], q.v[k]);
  }
  __device__ __forceinline__ Part part() const {
    Part q;
#pragma unroll
    for (int k = 0; k < VEC; ++k) q.v[k] = acc[k];
    return q;
  }
  // sum with the bias scaled by a per-row 0 / 1 flag (k_agg_flat XM 1): o + b * 1
  // is o + b bit for bit; o + b * 0 is o (a -0 row reads +0: equal values)
  __device__ __forceinline__ void finish_scaled_bias(const AggArgs& p, int64_t row, int64_t cnt, int f, bool act,
                                                     float bs) {
    if (!act) return;
    Frag<VEC> o;
    float c = (float)(cnt > 0 ? cnt : 1);
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = MEAN ? __fdiv_rn(acc[k], c) : acc[k];
    if (p.bias) {
      Frag<VEC> b = bias_of(p, f);
#pragma unroll
      for (int k = 0; k < VEC; ++k) o.v[k] = __fadd_rn(o.v[k], __fmul_rn(b.v[k], bs));
    }
    store_out<VEC>(p.out + row * p.ldo + f, o);
  }
  __device__ __forceinline__ void finish(const AggArgs& p, int64_t row, int64_t cnt, int f, bool act, bool with_bias = true) {
    if (!act) return;
    Frag<VEC> o;
    float c = (float)(cnt > 0 ? cnt : 1);
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = MEAN ? __fdiv_rn(acc[k], c) : acc[k];
    if (p.bias && with_bias) {
      Frag<VEC> b = bias_of(p, f);
#pragma unroll
      for (int k = 0; k < VEC; ++k) o.v[k] = __fadd_rn(o.v[k], b.v[k]);
    }
    store_out<VEC>(p.out + row * p.ldo + f, o);
  }
};

// torch_scatter CPU scatter_max/min [U9]: out starts at lowest()/max(),
// arg at src.size(0); strict compare so the FIRST edge (in original order)
// wins ties; afterwards out==init -> 0 (only when out was not passed in).
// Partials are merged in task order with the same strict compare: a later
// task only holds later edges of the row, so the first maximum survives.
template <int VEC, bool HAS_W, bool IS_MAX>
struct ArgRed : RedFlags {
  static constexpr bool kW = HAS_W;
  static constexpr bool kEid = true;
  struct Part {
    float v[VEC];
    int a[VEC];
  };
  float m[VEC];
  int a[VEC];
  int h = 0;
  int sentinel;

  __device__ ArgRed() {}
  __device__ ArgRed(const AggArgs& p, int, bool) : sentinel((int)p.n_ids) {}

  static __device__ __forceinline__ float init_val() { return IS_MAX ? -FLT_MAX : FLT_MAX; }
  static __device__ __forceinline__ bool better(float v, float cur) { return IS_MAX ? (v > cur) : (v < cur); }

  __device__ __forceinline__ void begin(const AggArgs& p, int64_t row, bool owned, int f, bool act) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      m[k] = init_val();
      a[k] = sentinel;
    }
    if (owned && (p.flags & MP_FLAG_INIT_FROM_OUT) && act) {
      Frag<VEC> o = load_frag<VEC>(p.out + row * p.ldo + f);
#pragma unroll
      for (int k = 0; k < VEC; ++k) m[k] = o.v[k];
    }
  }
  __device__ __forceinline__ void consume(const Frag<VEC>& v, float wt, int e, float) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float val = HAS_W ? __fmul_rn(wt, v.v[k]) : v.v[k];
      if (better(val, m[k])) {
        m[k] = val;
        a[k] = e;
      }
    }
  }
  __device__ __forceinline__ void save(PRef r, bool) const {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      r.v[k] = m[k];
      r.a[k] = a[k];
    }
  }
  static __device__ __forceinline__ Part load(PRef r) {
    Part q;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      q.v[k] = r.v[k];
      q.a[k] = r.a[k];
    }
    return q;
  }
  __device__ __forceinline__ void set(const Part& q) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      m[k] = q.v[k];
      a[k] = q.a[k];
    }
  }
  __device__ __forceinline__ void merge(const Part& q) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (better(q.v[k], m[k])) {
        m[k] = q.v[k];
        a[k] = q.a[k];
      }
    }
  }
  __device__ __forceinline__ Part part() const {
    Part q;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      q.v[k] = m[k];
      q.a[k] = a[k];
    }
    return q;
  }
  __device__ __forceinline__ void finish(const AggArgs& p, int64_t row, int64_t, int f, bool act, bool with_bias = true) {
    if (!act) return;
    Frag<VEC> o;
    const bool from_out = (p.flags & MP_FLAG_INIT_FROM_OUT) != 0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float v = m[k];
      if (!from_out && v == init_val()) v = 0.f;
      if (p.flags & MP_FLAG_PYG_MASK) {
        if (IS_MAX ? (v < -10000.f) : (v > 10000.f)) v = 0.f;
      }
      if (p.bias) v = __fadd_rn(v, p.bias[f + k]);
      o.v[k] = v;
    }
    store_out<VEC>(p.out + row * p.ldo + f, o);
    int64_t* ao = p.arg_out + row * (int64_t)p.F + f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) ao[k] = (int64_t)a[k];
  }
};

// Two-pass GAT (mp_gat_softmax_aggregate_f32): utils.softmax's row statistics
// [U3] as their own merge-path passes over x = a_src [N, H] (F = H, one lane
// task per row holding every head, k_agg_lane), then the aggregation as a
// weighted sum whose weights are the reference's alpha.
//   pass 1 (GatMaxRed): m[r,h]   = max_k leaky(a_src[col_k,h] + a_dst[r,h])
//   pass 2 (GatDenRed): den[r,h] = sum_k exp(leaky(.) - m[r,h]) + 1e-16, in
//                       CSR (= original edge) order, separately rounded
// Both write row_stats[r, h, 0|1] (the layout mp_gat_aggregate_f32 leaves).
// This GAT path lives with the plain aggregation, not in mp_gat_fwd.hip: its
// aggregation is the GA instance of k_agg_flat, and its fix-up is a
// k_agg_fixup<SumRed<..>> instance the plain dispatch already makes.
__device__ __forceinline__ float gat_leaky(float a, float slope) { return a > 0.f ? a : __fmul_rn(a, slope); }

template <int VEC>
struct GatMaxRed : RedFlags {
  struct Part {
    float v[VEC];
  };
  float acc[VEC];
  float ad[VEC];
  float slope = 0.f;
  int h = 0;  // slab_ref: no softmax-stat slab

  __device__ GatMaxRed() {}
  __device__ GatMaxRed(const AggArgs& p, int, bool) : slope(p.slope) {}

  __device__ __forceinline__ void begin(const AggArgs& p, int64_t row, bool, int f, bool act) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      acc[k] = -INFINITY;
      ad[k] = (act && f + k < p.F) ? p.a_dst[row * p.H + f + k] : 0.f;
    }
  }
  __device__ __forceinline__ void consume(const Frag<VEC>& v, float, int, float) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = fmaxf(acc[k], gat_leaky(__fadd_rn(v.v[k], ad[k]), slope));
  }
  __device__ __forceinline__ void save(PRef r, bool) const {
    Frag<VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = acc[k];
    store_frag<VEC>(r.v, o);
  }
  static __device__ __forceinline__ Part load(PRef r) {
    Frag<VEC> o = load_frag<VEC>(r.v);
    Part q;
#pragma unroll
    for (int k = 0; k < VEC; ++k) q.v[k] = o.v[k];
    return q;
  }
  __device__ __forceinline__ void set(const Part& q) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = q.v[k];
  }
  __device__ __forceinline__ void merge(const Part& q) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = fmaxf(acc[k], q.v[k]);
  }
  __device__ __forceinline__ Part part() const {
    Part q;
#pragma unroll
    for (int k = 0; k < VEC; ++k) q.v[k] = acc[k];
    return q;
  }
  __device__ __forceinline__ void finish(const AggArgs& p, int64_t row, int64_t, int f, bool act, bool with_bias = true) {
    if (!act) return;
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      if (f + k < p.F) p.row_stats[(row * p.H + f + k) * 2] = acc[k];
  }
};

template <int VEC>
struct GatDenRed : GatMaxRed<VEC> {
  using Base = GatMaxRed<VEC>;
  using typename Base::Part;
  using Base::acc;
  using Base::ad;
  using Base::slope;
  float m[VEC];

  __device__ GatDenRed() {}
  __device__ GatDenRed(const AggArgs& p, int f, bool act) : Base(p, f, act) {}

  __device__ __forceinline__ void begin(const AggArgs& p, int64_t row, bool, int f, bool act) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const bool ok = act && f + k < p.F;
      acc[k] = 0.f;
      ad[k] = ok ? p.a_dst[row * p.H + f + k] : 0.f;
      m[k] = ok ? p.row_stats[(row * p.H + f + k) * 2] : 0.f;
    }
  }
  __device__ __forceinline__ void consume(const Frag<VEC>& v, float, int, float) {
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      acc[k] = __fadd_rn(acc[k], expf(__fsub_rn(gat_leaky(__fadd_rn(v.v[k], ad[k]), slope), m[k])));
  }
  __device__ __forceinline__ void merge(const Part& q) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = __fadd_rn(acc[k], q.v[k]);
  }
  __device__ __forceinline__ void finish(const AggArgs& p, int64_t row, int64_t, int f, bool act, bool with_bias = true) {
    if (!act) return;
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      if (f + k < p.F) p.row_stats[(row * p.H + f + k) * 2 + 1] = __fadd_rn(acc[k], 1e-16f);
  }
};

// Per-head weighted sum (GAT backward: d out / d x_j = alpha[e,h]): the weight
// of slot k for this lane's head h = f / C is w[k*H + h].
template <int VEC>
struct HeadSumRed : SumRed<VEC, true, false> {
  static constexpr bool kW = false;
  static constexpr bool kHW = true;
  int h;
  __device__ HeadSumRed(const AggArgs& p, int f, bool act) : SumRed<VEC, true, false>(p, f, act),
                                                              h(act ? f / p.C : 0) {}
};

// Two-pass GAT aggregation window (k_agg_flat, 64-lane tasks, 64-feature
// tiles): lane k computes the reference's alpha for slot base+k and each of the
// hpt heads of this tile once per window,
//   alpha = exp(leaky(a_src[col,h] + a_dst[r,h]) - m[r,h]) / den[r,h],  r = slot_row,
// into the wave's LDS; a slot then costs one LDS read per lane (lane's head =
// its feature / C).  Columns and slot rows run two windows ahead and the
// per-slot gathers (a_src, a_dst, row stats) one window ahead.
struct GatAlphaWin {
  int64_t base, limit;
  int col, col_n, col_nn, row_n, row_nn;
  float g_as[4], g_ad[4], g_m[4], g_d[4];
  float* lds;
  int h0, hpt, j;

  __device__ __forceinline__ void fetch(const AggArgs& p, int64_t b, int lane, int& c, int& r) {
    const int64_t k = b + lane;
    const bool ok = k < limit;
    c = ok ? ld_stream(p.col + k) : 0;
    r = ok ? ld_stream(p.slot_row + k) : 0;
  }
  __device__ __forceinline__ void gather(const AggArgs& p, int c, int r) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < hpt) {
        const int64_t hr = (int64_t)r * p.H + h0 + q;
        g_as[q] = p.a_src[(int64_t)c * p.H + h0 + q];
        g_ad[q] = p.a_dst[hr];
        const f32x2 st = *reinterpret_cast<const f32x2*>(p.row_stats + hr * 2);
        g_m[q] = st.x;
        g_d[q] = st.y;
      }
    }
  }
  __device__ __forceinline__ void publish(const AggArgs& p, int lane) {
    float al[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      al[q] = q < hpt ? __fdiv_rn(expf(__fsub_rn(gat_leaky(__fadd_rn(g_as[q], g_ad[q]), p.slope), g_m[q])), g_d[q])
                      : 0.f;
    __builtin_amdgcn_wave_barrier();  // earlier reads of the previous window come first
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < hpt) lds[lane * hpt + q] = al[q];
    __builtin_amdgcn_wave_barrier();  // LDS ops of one wave run in order: later reads see the stores
  }
  __device__ __forceinline__ void init(const AggArgs& p, int64_t b, int64_t lim, int lane, float* wave_lds,
                                       int tile) {
    base = b;
    limit = lim;
    lds = wave_lds;
    // tile t holds features [64t, 64t+64): heads h0 .. h0+hpt-1, lane's head h0 + lane/C
    h0 = tile * 64 / p.C;
    hpt = p.C >= 64 ? 1 : min(64 / p.C, p.H - h0);  // a last partial tile holds fewer heads
    j = p.C >= 64 ? 0 : lane / p.C;                  // lanes past F read some slot's alpha, unused
    int r;
    fetch(p, base, lane, col, r);
    fetch(p, base + 64, lane, col_n, row_n);
    fetch(p, base + 128, lane, col_nn, row_nn);
    gather(p, col, r);
    publish(p, lane);
    gather(p, col_n, row_n);
  }
  __device__ __forceinline__ void ensure(const AggArgs& p, int64_t e, int lane) {
    if (e >= base + 64) {  // slots are consumed in order, never skipping a window
      base += 64;
      col = col_n;
      publish(p, lane);  // the gathers issued a window ago
      col_n = col_nn;
      row_n = row_nn;
      fetch(p, base + 128, lane, col_nn, row_nn);
      gather(p, col_n, row_n);
    }
  }
  __device__ __forceinline__ float alpha(int slot_in_win) const { return lds[slot_in_win * hpt + j]; }
};

// ---------------------------------------------------------------------------
// Narrow rows (F <= 16): one merge-path task per LANE.  A lane holds the whole
// row (NV fragments of VEC features, one reducer each) and walks its task's
// slots in CSR order with U slots' loads in flight, so a wave keeps 64*U row
// gathers outstanding instead of 64/L*L.  Same schedule, slab layout and
// fix-up as k_agg_main; rows stay sequential, so results are identical.
// ---------------------------------------------------------------------------
template <class Red, int VEC, int NV, int U>
__device__ __forceinline__ void lane_slots(Red (&red)[NV], const AggArgs& p, int64_t s, int64_t t) {
  for (int64_t e = s; e < t; e += U) {
    const int64_t n = t - e < U ? t - e : U;
    int c[U];
    [[maybe_unused]] float wt[U];
    [[maybe_unused]] int ei[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t k = e + (u < n ? u : n - 1);
      c[u] = p.col ? p.col[k] : (int)k;
      if constexpr (Red::kW) wt[u] = p.w[k];
      if constexpr (Red::kEid) ei[u] = p.eid[k];
    }
    Frag<VEC> v[U][NV];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float* row = p.x + (int64_t)c[u] * p.ldx;
#pragma unroll
      for (int q = 0; q < NV; ++q) v[u][q] = load_frag<VEC>(row + (q * VEC < p.F ? q * VEC : 0));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < n) {
#pragma unroll
        for (int q = 0; q < NV; ++q)
          red[q].consume(v[u][q], Red::kW ? wt[u] : 1.f, Red::kEid ? ei[u] : 0, 0.f);
      }
    }
  }
}

template <class Red, int VEC, int NV, int U>
__global__ __launch_bounds__(kBlock) void k_agg_lane(AggArgs p) {
  const int w = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (w >= p.n_waves) return;
  const int r_first = p.wave_row[w];
  const int r_last = p.wave_row[w + 1];
  const int64_t e_begin = p.wave_slot[w];
  const int64_t e_end = p.wave_slot[w + 1];
  Red red[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) red[q] = Red(p, q * VEC, q * VEC < p.F);
  const int64_t ce = p.rowptr[r_first];
  if (e_begin < ce) {
#pragma unroll
    for (int q = 0; q < NV; ++q) red[q].begin(p, r_first - 1, false, q * VEC, q * VEC < p.F);
    lane_slots<Red, VEC, NV, U>(red, p, e_begin, ce < e_end ? ce : e_end);
#pragma unroll
    for (int q = 0; q < NV; ++q)
      if (q * VEC < p.F) red[q].save(slab_ref(p, 2 * (int64_t)w, q * VEC, red[q]), false);
  }
  int64_t rs = ce;
  for (int r = r_first; r < r_last; ++r) {
    const int64_t re = p.rowptr[r + 1];
#pragma unroll
    for (int q = 0; q < NV; ++q) red[q].begin(p, r, true, q * VEC, q * VEC < p.F);
    if (re <= e_end) {
      lane_slots<Red, VEC, NV, U>(red, p, rs, re);
#pragma unroll
      for (int q = 0; q < NV; ++q) red[q].finish(p, r, re - rs, q * VEC, q * VEC < p.F);
    } else {
      lane_slots<Red, VEC, NV, U>(red, p, rs, e_end);
#pragma unroll
      for (int q = 0; q < NV; ++q)
        if (q * VEC < p.F) red[q].save(slab_ref(p, 2 * (int64_t)w + 1, q * VEC, red[q]), false);
    }
    rs = re;
  }
}

// ---------------------------------------------------------------------------
// Flat variant of k_agg_main (sum/mean/max/min): a task streams its slots in
// fixed batches of U across row boundaries and closes rows as it crosses
// their ends (row ends come from the rowptr window already in registers).
// k_agg_main starts a new batch at every row, so a short row costs a whole
// batch of U (clamped) loads and a trip of loop overhead; here every batch
// but the task's last carries U useful slots, and the next row's loads are
// in flight while the previous row is finished.  Each row's slots are still
// consumed in CSR order by one task: results are identical.
// ---------------------------------------------------------------------------
// GA: two-pass GAT aggregation (Red = SumRed<1, true, false>, L = 64): the slot
// weights are the reference's alpha from GatAlphaWin instead of w.
// SM (L = 64, no edge ids, col != nullptr, x below 4 GiB): the column and
// weight of every slot of a batch come straight into SGPRs through scalar
// loads (s_load_dwordx16 via the scalar cache) -- the next batch's columns
// issued with the current batch, the current batch's weights consumed only
// after its gathers are in flight -- and each gather is a buffer load with the
// row offset in soffset: per slot one SALU multiply and one VMEM instruction,
// no v_readlane from a one-slot-per-lane window.
template <int U, class T>
__device__ __forceinline__ void scalar_batch(const T* a, int64_t n, int64_t e, T (&v)[U]) {
  typedef T tv __attribute__((ext_vector_type(U), aligned(4)));
  typedef __attribute__((address_space(4))) const tv ctv;
  typedef __attribute__((address_space(4))) const T ct;
  // slots [e, e + U); slots past the end of the array are clamped to the last
  // one (never consumed: the caller stops at the task's end)
  if (e + U <= n) {
    const tv t = *(ctv*)(a + e);
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = t[u];
  } else {
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ((ct*)a)[batch_slot(e, u, n)];
  }
}

// MP_FLAG_SKIP_EMPTY (mp_aggregate_tiles_f32 only): an owned row with no slot
// is left untouched -- no load, no store, no bias.  The sharded step's boundary
// pass (INIT_FROM_OUT) skips its rows without boundary edges this way: their
// read-modify-write of out cost the pass as much as its gathers (measured,
// tools/exp_boundary.py), and the interior pass adds their bias instead
// (AggArgs::bias_rows).  (An out prefetch issued with each batch's gathers was
// also measured there: slower, not kept -- DESIGN Appendix A.)
// XM (mp_aggregate_tiles_f32's launches only): 1 = per-row bias flags (the
// sharded interior pass), 2 = MP_FLAG_SKIP_EMPTY (the boundary pass); TM:
// tile-major operands.  Compile-time, one feature per instance, so every other
// launch runs the kernel without their per-block and per-row work (measured:
// both features as run-time branches of one instance cost short-row passes 13 %).
// Ring depth of the scalar-batch loop's rolling gather window, per family of
// launches; 0: batches of U issued and consumed whole, the loop as it was
// before the window.  U stays the instance's name.  Measured (main kernel,
// bitwise-equal outputs; DESIGN Appendix A):
//  * x beyond the Infinity Cache, plain operands (config 2 / config 5): a ring
//    of 4 runs 6.33 / 14.06 ms against 6.57 / 14.65 ms for batches of 8.  With
//    the ring still draining at every row's end, rings of 2, 3, 4, 5, 6 and 8
//    ran 8.21, 7.21, 6.45, 6.55, 6.77 and 6.97 ms on config 2;
//  * the sharded step's far tile launches without per-row options run this
//    same instance: interior 0.238 -> 0.202 ms, send packing 0.643 -> 0.614,
//    boundary pull unchanged (tools/exp_interior.py);
//  * the XM != 0 and tile-major instances keep whole batches: rings of 4 and 8
//    lost 2 - 5 % on some pass each when measured with the row-end drain
//    still in; not measured again without it;
//  * x inside the Infinity Cache (U = 16): a ring of 16 ran 2.76 ms against
//    3.03 ms at Reddit scale (with the drain); not switched on, the tile
//    launches that share the instance are not measured.
template <int VEC, int U, int XM, bool TM>
constexpr int flat_ring() {
  return (VEC == 1 && U == kU_Vec1Far && XM == 0 && !TM) ? 4 : 0;
}

template <class Red, int VEC, int U, int L, bool GA = false, bool SM = false, int XM = 0, bool TM = false>
__global__ __launch_bounds__(kBlock) void k_agg_flat(AggArgs p) {
  static_assert(!Red::kGat && !Red::kGatB && !Red::kHW, "flat loop: sum/mean/max/min reducers");
  static_assert(!GA || (L == 64 && VEC == 1 && Red::kW), "two-pass GAT: 64-lane tasks, 64-feature tiles");
  static_assert(!SM || (L == 64 && !GA && !Red::kEid), "scalar batches: 64-lane sum/mean tasks");
  static_assert(!(XM || TM) || (SM && VEC == 1), "tile-major / skipped rows: the scalar-batch kernel, 64-feature tiles");
  constexpr bool kSkip = XM == 2, kFlags = XM == 1;
  constexpr int R = SM ? flat_ring<VEC, U, XM, TM>() : 0;  // rolling gather window of R entries
  constexpr bool kRoll = R > 0;
  constexpr int B = kRoll ? R : U;                     // slots per scalar batch
  using GR = Grp<L>;
  const int lane = lane_id();
  const int gl = lane & (L - 1);
  int bx = (int)blockIdx.x, tile = (int)blockIdx.y;
  if constexpr (kXcdTiles) {  // see k_agg_main: one feature tile per XCD
    const int T = (int)gridDim.y;
    if (8 % T == 0 && !p.seq_tiles) {  // the host pads the grid to a multiple of 8/T blocks per tile
      const int b = (int)(blockIdx.y * gridDim.x + blockIdx.x);
      const int xcd = b & 7;
      tile = xcd % T;
      bx = (b >> 3) * (8 / T) + xcd / T;
    }
  }
  const int wave = bx * kWavesPerBlock + (int)(threadIdx.x >> 6);
  const int w = GR::un(wave * GR::G + lane / L);
  if (w >= p.n_waves) return;
  const int f = tile * L * VEC + gl * VEC;
  const bool act = f < p.F;
  const float* x_tile = p.x;
  int64_t ldx_tile = p.ldx;
  int fx0 = 0;
  if constexpr (TM) tile_view(p, tile * L * VEC, x_tile, ldx_tile, fx0);
  const uint32_t foff = (uint32_t)(act ? f - fx0 : 0) * 4u;
  const char* xb = reinterpret_cast<const char*>(x_tile);
  const int64_t ldxb = ldx_tile * 4;
  [[maybe_unused]] __amdgpu_buffer_rsrc_t xr;


  const int r_first = GR::un(p.wave_row[w]);
  const int r_last = GR::un(p.wave_row[w + 1]);
  const int64_t e_begin = GR::un(p.wave_slot[w]);
  const int64_t e_end = GR::un(p.wave_slot[w + 1]);

  Red red(p, f, act);
  // the tile launches, and the rolling window (sum / mean only): a bias load per
  // row would drain the gather ring at every row's end (config 2, ring of 4:
  // 6.79 ms with the load per row, 6.45 ms with it per task)
  if constexpr (XM != 0 || kRoll) red.preload_bias(p, f, act);
  // a row's accumulator starts (the rolling window: with its initial value landed)
  auto begin_row = [&](int64_t rr, bool owned) {
    if constexpr (kRoll) red.template begin_at<true>(p, rr, owned, f, act);
    else red.begin(p, rr, owned, f, act);
  };
  // an owned row opens (rs_ / re_: its slot range); an empty one is skipped
  // (no load of out) under MP_FLAG_SKIP_EMPTY
  auto open_row = [&](int rr, int64_t rs_, int64_t re_) { begin_row(rr, !(kSkip && re_ == rs_)); };

  std::conditional_t<GA, GatAlphaWin, SlotWin<Red::kW, Red::kEid, L>> win;
  if constexpr (GA) {
    __shared__ float ga_lds[kWavesPerBlock][64 * 4];
    win.init(p, e_begin, e_end, gl, ga_lds[threadIdx.x >> 6], tile);
  } else if constexpr (!SM) {
    win.init(p, e_begin, e_end, gl);
  }
  [[maybe_unused]] int c_nxt[B];
  if constexpr (SM) {
    xr = __builtin_amdgcn_make_buffer_rsrc((void*)x_tile, (short)0, (int)p.x_bytes, 0x00020000);
    if (e_begin < e_end) scalar_batch<B>(p.col, p.n_edges, e_begin, c_nxt);
  }
  // row window: rowptr (and, kFlags, the per-row bias flags) of rows [rbase,
  // rbase + L) across the lanes.  A kFlags refill for row pointer r starts at
  // r - 1, so the row that r closes -- the one open -- stays in the window
  // until it finishes (its bias flag is read then).
  int rbase = r_first;
  int rp = (rbase + gl <= p.n_rows) ? p.rowptr[rbase + gl] : 0;
  [[maybe_unused]] int bw = 1;
  if constexpr (kFlags) bw = (rbase + gl < p.n_rows) ? p.bias_rows[rbase + gl] : 1;
  auto row_ptr = [&](int r) -> int64_t {
    if (r - rbase > L - 1) {
      rbase = kFlags ? r - 1 : r;
      rp = (rbase + gl <= p.n_rows) ? p.rowptr[rbase + gl] : 0;
      if constexpr (kFlags) bw = (rbase + gl < p.n_rows) ? p.bias_rows[rbase + gl] : 1;
      // the rolling window: the refill is waited for here, once per 64 rows.  Left
      // pending, it puts an s_waitcnt vmcnt(0) in front of the v_readlane below on
      // every path, and the ring drains at every row's end.
      if constexpr (kRoll) asm volatile("" : "+v"(rp));
    }
    return GR::bc(rp, r - rbase);
  };
  auto finish_row = [&](int rr, int64_t cnt) {
    if constexpr (kSkip) {
      if (cnt == 0) return;
    }
    if constexpr (kFlags) {
      red.finish_scaled_bias(p, rr, cnt, f, act, GR::bc(bw, rr - rbase) != 0 ? 1.f : 0.f);
    } else {
      red.finish(p, rr, cnt, f, act);
    }
  };

  // current row: the continuation of an earlier task's row, or an owned row
  const int64_t ce = GR::bc(rp, 0);  // rowptr[r_first]
  bool cont = e_begin < ce;
  int r = r_first;
  int64_t rs = ce, re = ce;
  if (cont) {
    begin_row(r_first - 1, false);
  } else if (r < r_last) {
    re = row_ptr(r + 1);
    open_row(r, rs, re);
  }
  // close the current row at slot k (k >= its end) and open the next one(s)
  auto advance = [&](int64_t k) {
    while (k >= re) {
      if (cont) {
        if (act) red.save(slab_ref(p, 2 * (int64_t)w, f, red), false);
        cont = false;
      } else {
        finish_row(r, re - rs);
        ++r;
      }
      if (r >= r_last) {  // cannot happen for a valid schedule: never open a row past the task
        re = INT64_MAX;
        break;
      }
      rs = re;
      re = row_ptr(r + 1);
      open_row(r, rs, re);
    }
  };

  if constexpr (kRoll) {
    // Rolling gather window (mp_flat_ring.h): a ring of R gathers.  Every batch
    // but the task's last refills entry u with slot e + R + u as soon as slot
    // e + u is consumed, so the wave keeps R - 1 .. R gathers in flight until
    // the task's last batch instead of draining to none at the end of every
    // batch.  Batches start at e_begin + k*R.  The refills of batch k read the
    // columns of batch k + 1 (c_nxt); once the last of them is issued, the
    // columns of batch k + 2 and the weights of batch k + 1 are loaded into the
    // same SGPRs, and land while batch k + 1 waits for its first row, R - 1
    // gathers behind it.  (A second SGPR set for each, loaded a batch earlier,
    // took the kernel from 88 to 106 SGPRs: one resident block per CU fewer.)
    // The refills are unconditional: a refill under a per-slot condition is
    // loaded into a temporary and copied behind an s_waitcnt vmcnt(0).  Those
    // of the last-but-one batch that fall past e_end are never consumed, like
    // the tail of the last batch's loads before.  Slots are consumed in the
    // same order as ever.
    Frag<VEC> v[R];
    [[maybe_unused]] float w_cur[R];
    int64_t e = e_begin;
    if (e < e_end) {
#pragma unroll
      for (int u = 0; u < R; ++u) v[u] = load_frag_buf<VEC>(xr, foff, (uint32_t)c_nxt[u] * (uint32_t)ldxb);
      if (ring_refills(e, e_end, R)) scalar_batch<R>(p.col, p.n_edges, e + R, c_nxt);
      if constexpr (Red::kW) scalar_batch<R>(p.w, p.n_edges, e, w_cur);
    }
    for (; ring_refills(e, e_end, R); e += R) {
#pragma unroll
      for (int u = 0; u < R; ++u) {
        advance(e + u);
        float wt = 1.f;
        if constexpr (Red::kW) wt = w_cur[u];
        red.consume(v[u], wt, 0, 0.f);
        red.pin();
        v[u] = load_frag_buf<VEC>(xr, foff, (uint32_t)c_nxt[u] * (uint32_t)ldxb);
      }
      if (ring_loads_cols(e, e_end, R)) scalar_batch<R>(p.col, p.n_edges, e + 2 * R, c_nxt);
      if constexpr (Red::kW) scalar_batch<R>(p.w, p.n_edges, e + R, w_cur);
    }
    if (e < e_end) {
      const int n = ring_last(e, e_end);
#pragma unroll
      for (int u = 0; u < R; ++u) {
        if (u < n) {
          advance(e + u);
          float wt = 1.f;
          if constexpr (Red::kW) wt = w_cur[u];
          red.consume(v[u], wt, 0, 0.f);
        }
      }
    }
  }
  if constexpr (!kRoll) for (int64_t e = e_begin; e < e_end;) {
    if constexpr (SM) {
      // batches start at e_begin + k*U: every batch but the task's last is full
      const int64_t rem = e_end - e;
      const int n = rem < U ? (int)rem : U;
      [[maybe_unused]] float wb[U];
      if constexpr (Red::kW) scalar_batch<U>(p.w, p.n_edges, e, wb);
      Frag<VEC> v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = load_frag_buf<VEC>(xr, foff, (uint32_t)c_nxt[u] * (uint32_t)ldxb);
      // the columns are dead once the gathers are issued: the next batch's
      // land in the same SGPRs while this batch's rows are in flight
      if (e + U < e_end) scalar_batch<U>(p.col, p.n_edges, e + U, c_nxt);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (u < n) {
          advance(e + u);
          float wt = 1.f;
          if constexpr (Red::kW) wt = wb[u];
          red.consume(v[u], wt, 0, 0.f);
        }
      }
      e += n;
      continue;
    }
    win.ensure(p, e, gl);
    const int off = (int)(e - win.base);
    int64_t rem = e_end - e;
    int n = L - off;
    if (rem < n) n = (int)rem;
    if (n > U) n = U;
    n = GR::un(n);
    Frag<VEC> v[U];
    [[maybe_unused]] float al[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int uu = u < n ? u : n - 1;
      const int c = GR::bc(win.col, off + uu);
      v[u] = load_frag<VEC>(reinterpret_cast<const float*>(xb + (int64_t)c * ldxb + foff));
      if constexpr (GA) al[u] = win.alpha(off + uu);  // LDS reads of the batch issued with its loads
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < n) {
        advance(e + u);
        float wt = 1.f;
        if constexpr (GA) wt = al[u];
        else if constexpr (Red::kW) wt = GR::bc(win.w, off + u);
        int ei = 0;
        if constexpr (!GA && Red::kEid) ei = GR::bc(win.eid, off + u);
        red.consume(v[u], wt, ei, 0.f);
      }
    }
    e += n;
  }
  // tail: the current row, then any rows whose slots all lie in later tasks
  if (cont) {
    if (act) red.save(slab_ref(p, 2 * (int64_t)w, f, red), false);
    cont = false;
    if (r < r_last) {
      rs = ce;
      re = row_ptr(r + 1);
      open_row(r, rs, re);
    }
  }
  while (r < r_last) {
    if (re <= e_end) {
      finish_row(r, re - rs);
    } else {
      if (act) red.save(slab_ref(p, 2 * (int64_t)w + 1, f, red), false);
    }
    ++r;
    if (r < r_last) {
      rs = re;
      re = row_ptr(r + 1);
      open_row(r, rs, re);
    }
  }
}

// the same reducer at another lane width (fix-up of a VEC < 4 flat kernel at VEC=4)
template <class Red, int V>
struct Rebind {
  using type = Red;
};
template <int VEC, bool W, bool M, int V>
struct Rebind<SumRed<VEC, W, M>, V> {
  using type = SumRed<V, W, M>;
};
template <int VEC, bool W, bool M, int V>
struct Rebind<ArgRed<VEC, W, M>, V> {
  using type = ArgRed<V, W, M>;
};

// What choose() settled about one sum / mean / max / min launch besides the
// reducer and the lane shape; the ladder below turns it into kernels.
struct FlatChoice {
  bool flat = false;   // run k_agg_flat instead of k_agg_main (64-lane tasks)
  bool smem = false;   // flat sum/mean kernel: slot columns/weights through scalar loads (k_agg_flat SM)
  bool far = false;    // flat SM kernel: x larger than the Infinity Cache (batches of kU_Vec1Far)
  bool tiles = false;  // mp_aggregate_tiles_f32: the SM kernel's XM / TM instance (tile-major operands,
                       // skipped rows, per-row bias)
  bool fixup4 = false; // VEC < 4 flat kernel: run the fix-up at VEC=4 (slabs are indexed by feature)
};

// the mp_aggregate_tiles_f32 instances: XM from the call (per-row bias flags /
// skipped rows / neither), TM when an operand is tile-major
template <class Red, int U, int XM>
static AggKernel flat_xm(const AggArgs& a, bool far) {
  const bool tm = a.x_tw || a.o_tw;
  if (tm)
    return far ? k_agg_flat<Red, 1, kU_Vec1Far, 64, false, true, XM, true>
               : k_agg_flat<Red, 1, U, 64, false, true, XM, true>;
  return far ? k_agg_flat<Red, 1, kU_Vec1Far, 64, false, true, XM> : k_agg_flat<Red, 1, U, 64, false, true, XM>;
}
template <class Red, int U>
static AggKernel flat_tiles(const AggArgs& a, bool far) {
  if (a.bias_rows) return flat_xm<Red, U, 1>(a, far);
  if (a.flags & MP_FLAG_SKIP_EMPTY) return flat_xm<Red, U, 2>(a, far);
  return flat_xm<Red, U, 0>(a, far);
}

// The k_agg_flat instance of one launch (64-lane tasks): its smem / far / tile
// instances for sum and mean, the slot window for max and min.
template <class Red, int VEC>
static AggKernel flat_kernel(const AggArgs& a, const FlatChoice& c) {
  constexpr int U = kMainU<Red, VEC, 64>;
  if constexpr (!Red::kEid) {
    if constexpr (VEC == 1) {
      const bool far = c.smem && c.far;
      // mp_aggregate_tiles_f32 (scalar batches, 64-feature tiles by construction)
      if (c.tiles) return flat_tiles<Red, U>(a, far);
      if (far) return k_agg_flat<Red, 1, kU_Vec1Far, 64, false, true>;
    }
    if (c.smem) return k_agg_flat<Red, VEC, U, 64, false, true>;
  }
  return k_agg_flat<Red, VEC, U, 64>;
}

template <class Red, int VEC, int NV>
static AggLaunch lane_launch(const AggArgs& a) {
  constexpr int U = VEC * NV >= 16 ? (kULane + 1) / 2 : kULane;  // 16-float rows: keep VGPRs < 128
  return with_fixup<Red, VEC>(k_agg_lane<Red, VEC, NV, U>, dim3((unsigned)ceil_div(a.n_waves, kBlock)), a);
}

// One sum / mean / max / min launch of reducer Red at VEC features per lane:
// lane tasks for F <= kLaneMaxF (VEC=4 with NV in {1,2} or VEC=1 with NV in
// {4,8}), k_agg_flat where the choice is flat (under c.fixup4 with the fix-up at
// VEC = 4), else the engine's k_agg_main with `lanes`-lane tasks and its fix-up.
template <class Red, int VEC>
static AggLaunch launch_of(const AggArgs& a, const FlatChoice& c, int lanes) {
  if constexpr (VEC != 2) {
    if (a.F <= kLaneMaxF && a.F >= 2) {
      if constexpr (VEC == 4) return a.F <= 4 ? lane_launch<Red, 4, 1>(a) : lane_launch<Red, 4, 2>(a);
      else return a.F <= 4 ? lane_launch<Red, 1, 4>(a) : lane_launch<Red, 1, 8>(a);
    }
  }
  if (!c.flat) return engine_launch_at<Red, VEC>(lanes, a);
  const AggKernel k = flat_kernel<Red, VEC>(a, c);
  const dim3 grid = main_grid<VEC, 64>(a);
  if constexpr (VEC != 4) {
    if (c.fixup4) return with_fixup<typename Rebind<Red, 4>::type, 4>(k, grid, a);
  }
  return with_fixup<Red, VEC>(k, grid, a);
}

// reduce is one of the four (the callers checked)
template <int VEC>
static AggLaunch launch_of_reduce(const AggArgs& a, int reduce, const FlatChoice& c, int lanes) {
  const bool hw = a.w != nullptr;
  switch (reduce) {
    case MP_REDUCE_SUM:
      return hw ? launch_of<SumRed<VEC, true, false>, VEC>(a, c, lanes)
                : launch_of<SumRed<VEC, false, false>, VEC>(a, c, lanes);
    case MP_REDUCE_MEAN:
      return hw ? launch_of<SumRed<VEC, true, true>, VEC>(a, c, lanes)
                : launch_of<SumRed<VEC, false, true>, VEC>(a, c, lanes);
    case MP_REDUCE_MAX:
      return hw ? launch_of<ArgRed<VEC, true, true>, VEC>(a, c, lanes)
                : launch_of<ArgRed<VEC, false, true>, VEC>(a, c, lanes);
    default:  // MP_REDUCE_MIN
      return hw ? launch_of<ArgRed<VEC, true, false>, VEC>(a, c, lanes)
                : launch_of<ArgRed<VEC, false, false>, VEC>(a, c, lanes);
  }
}

// A statistics pass of the two-pass GAT over x = a_src [N, H] (F = H): k_agg_main
// lane groups, one lane per head: H <= 4 -> 4 lanes, <= 8 -> 8, else 16
template <class Red>
static AggLaunch gat_stats_launch(const AggArgs& t) {
  if (t.H <= 4) return engine_launch<Red, 1, 4>(t);
  if (t.H <= 8) return engine_launch<Red, 1, 8>(t);
  return engine_launch<Red, 1, 16>(t);
}

// ---------------------------------------------------------------------------
// mp_tune: the one table of run-time dispatch choices (include/mi355_mp.h).
// Defaults are the A/B winners; every alternative gives
// bitwise-identical results.
// ---------------------------------------------------------------------------
struct Tune {
  std::atomic<int64_t> flat_vec1_min_bytes{0};  // sum/mean: 64-feature tiles at every x size (scalar batches)
  std::atomic<int64_t> flat_smem{1};
  std::atomic<int64_t> flat_min_f{64};
  std::atomic<int64_t> flat_min_f_arg{64};
  std::atomic<int64_t> flat_narrow_vec1{64};  // F=64: one full 64-feature tile, -26% vs a half-used 128 tile
  std::atomic<int64_t> flat_vec{2};
  std::atomic<int64_t> flat_vec_arg{2};
  std::atomic<int64_t> flat_seq_tiles{0};
  std::atomic<int64_t> flat_far_min_bytes{256ll << 20};  // the Infinity Cache
  std::atomic<int64_t> gat_bwd_vec{4};  // features per lane of the GAT backward's transposed pass
  std::atomic<int64_t> topk_wg_limit{2048};  // largest graph mp_topk_select_f32 ranks in one workgroup (mp_pool.hip)
};
static Tune g_tune;

static std::atomic<int64_t>* tune_slot(int32_t key) {
  switch (key) {
    case MP_TUNE_FLAT_VEC1_MIN_BYTES: return &g_tune.flat_vec1_min_bytes;
    case MP_TUNE_FLAT_SMEM: return &g_tune.flat_smem;
    case MP_TUNE_FLAT_MIN_F: return &g_tune.flat_min_f;
    case MP_TUNE_FLAT_MIN_F_ARG: return &g_tune.flat_min_f_arg;
    case MP_TUNE_FLAT_NARROW_VEC1: return &g_tune.flat_narrow_vec1;
    case MP_TUNE_FLAT_VEC: return &g_tune.flat_vec;
    case MP_TUNE_FLAT_VEC_ARG: return &g_tune.flat_vec_arg;
    case MP_TUNE_FLAT_SEQ_TILES: return &g_tune.flat_seq_tiles;
    case MP_TUNE_FLAT_FAR_MIN_BYTES: return &g_tune.flat_far_min_bytes;
    case MP_TUNE_GAT_BWD_VEC: return &g_tune.gat_bwd_vec;
    case MP_TUNE_TOPK_WG_LIMIT: return &g_tune.topk_wg_limit;
  }
  return nullptr;
}

static inline int64_t tuned(std::atomic<int64_t>& v) { return v.load(std::memory_order_relaxed); }

int64_t tuned_gat_bwd_vec() { return tuned(g_tune.gat_bwd_vec); }
int64_t tuned_topk_wg_limit() { return tuned(g_tune.topk_wg_limit); }

// The kernels of one mp_aggregate_f32 call (tiles: of one mp_aggregate_tiles_f32
// call), args checked: a pure function of the arguments and the mp_tune table.
// It launches nothing; of `a` it sets the two fields the flat kernel reads on
// the device, x_bytes and seq_tiles.
static AggLaunch choose(AggArgs& a, const mp_csr* g, int reduce, bool tiles = false) {
  const int F = a.F;
  const bool is_arg = reduce == MP_REDUCE_MAX || reduce == MP_REDUCE_MIN;
  FlatChoice c;
  if (tiles) {
    // tile-major operands (mp_aggregate_tiles_f32, arguments checked there): the
    // scalar-batch flat kernel with 64-feature tiles, its fix-up 64 wide
    const int64_t xbytes = (int64_t)g->n_cols * (a.x_tw ? a.x_tw : a.ldx) * 4;
    c.flat = true;
    c.smem = true;
    a.x_bytes = (uint32_t)xbytes;
    c.far = xbytes > tuned(g_tune.flat_far_min_bytes);
    // feature tiles one after another when x outgrows the Infinity Cache by up to 4x: then
    // each 64-feature tile of it (a quarter) fits, and the tiles take turns in it (the
    // sharded step's P = 4 passes: interior 0.68 -> 0.65 ms, send 1.26 -> 1.22 ms; at P = 8,
    // x fits whole and XCD-affine tiles stay ahead by 1-2 %; tools/exp_boundary.py)
    const int64_t x_all = (int64_t)g->n_cols * F * 4;
    a.seq_tiles = (tuned(g_tune.flat_seq_tiles) || (x_all > kSeqTilesMin && x_all <= 4 * tuned(g_tune.flat_far_min_bytes)))
                      ? 1 : 0;
    c.tiles = true;
    return launch_of_reduce<1>(a, reduce, c, 64);
  }
  Shape sh = pick_shape(F, a.ldx, a.x, a.ldo, a.out);
  // flat kernel lane width: 64-feature tiles (VEC=1) for sum/mean, where an
  // XCD's L2 holding one narrow tile of the hot rows pays (Reddit-scale x of
  // 238 MB: 8.28 -> 7.25 ms; RMAT21 x of 2 GB 6.98 -> 6.73 ms); 128-feature
  // tiles (VEC=2) for max/min, whose compare-and-select per element is bound
  // by the texture-address unit rather than by L2 misses (VEC=1: +15..29%)
  const int64_t xbytes = (int64_t)g->n_cols * a.ldx * 4;
  int fvec = (int)(is_arg ? tuned(g_tune.flat_vec_arg) : tuned(g_tune.flat_vec));
  // The L1 miss queue holds 256-B segments: a 64-feature
  // tile of a row that does not start on a 256-B boundary straddles two of
  // them.  Such rows take the widest per-lane vector the layout allows, which
  // touches the fewest segments per row (F=200: 8.43 -> 6.93 ms sum, 8.34 ->
  // 7.16 ms max; F=130 sum 6.78 -> 6.44 ms on RMAT21).
  const bool seg_aligned = (a.ldx * 4) % 256 == 0 && (uintptr_t)a.x % 256 == 0;
  if (!seg_aligned) {
    fvec = sh.vec;
  } else {
    if (!is_arg && xbytes >= tuned(g_tune.flat_vec1_min_bytes)) fvec = 1;
    if (F <= tuned(g_tune.flat_narrow_vec1)) fvec = 1;
  }
  // sum/mean: slot columns and weights through scalar loads (k_agg_flat SM),
  // 32-bit buffer offsets (soffset + lane offset) while x spans < 4 GiB.
  // (Max/min through the same batches, edge ids included: bitwise equal and
  // no faster -- Reddit-scale 8.67 vs 8.67 ms, RMAT21 7.77 vs 7.76 ms,
  // profiles/r02_ab_smem_arg.log -- so they keep the slot window.)
  c.smem = tuned(g_tune.flat_smem) && !is_arg && a.col != nullptr && g->n_cols > 0 && xbytes <= 0xFFFFFFF0LL;
  if (c.smem) a.x_bytes = (uint32_t)xbytes;
  // In-flight depth of the scalar-batch kernel: 16 row loads per wave while x
  // fits the Infinity Cache (Reddit-scale, 238 MB: 7.25 ms vs 7.64 at 8); 8
  // beyond it (RMAT21 6.71 -> 6.58 ms, ogbn-products-scale 15.0 -> 14.6 ms;
  // profiles/r02_ab_batch_u.log)
  c.far = xbytes > tuned(g_tune.flat_far_min_bytes);
  a.seq_tiles = (int32_t)tuned(g_tune.flat_seq_tiles);
  const int64_t min_f = is_arg ? tuned(g_tune.flat_min_f_arg) : tuned(g_tune.flat_min_f);
  if (F >= min_f && F % fvec == 0 && sh.vec >= fvec) {
    sh.vec = fvec;  // narrow feature tiles, slot batches across rows
    sh.lanes = 64;
    c.flat = true;
    // the fix-up reads slabs by feature: run it 4 wide when out (and bias) allow
    c.fixup4 = F % 4 == 0 && (uintptr_t)a.out % 16 == 0 && a.ldo % 4 == 0 && (uintptr_t)a.bias % 16 == 0;
  }
  switch (sh.vec) {
    case 4: return launch_of_reduce<4>(a, reduce, c, sh.lanes);
    case 2: return launch_of_reduce<2>(a, reduce, c, 64);
    default: return launch_of_reduce<1>(a, reduce, c, 64);
  }
}

}  // namespace mp

using namespace mp;

extern "C" {

int64_t mp_tune(int32_t key, int64_t value) {
  std::atomic<int64_t>* v = tune_slot(key);
  if (!v) return -1;
  if (value < 0) return v->load();
  if (key == MP_TUNE_FLAT_SMEM || key == MP_TUNE_FLAT_SEQ_TILES) value = value ? 1 : 0;
  if ((key == MP_TUNE_FLAT_VEC || key == MP_TUNE_FLAT_VEC_ARG || key == MP_TUNE_GAT_BWD_VEC) && value != 1 &&
      value != 2 && value != 4)
    return -1;
  if (key == MP_TUNE_TOPK_WG_LIMIT && (value < 64 || value > 8192)) return -1;
  return v->exchange(value);
}

size_t mp_aggregate_slab_bytes(const mp_csr* g, int32_t F, int32_t reduce) {
  if (!g || F <= 0) return 256;
  bool arg = reduce == MP_REDUCE_MAX || reduce == MP_REDUCE_MIN;
  return slab_layout(g->n_waves, F, 0, arg ? kSlabArg : 0).total;
}

int mp_aggregate_f32(const mp_csr* g, const float* w, const float* x, int64_t ldx, int32_t F,
                     int32_t reduce, int32_t flags, const float* bias, float* out, int64_t ldo,
                     int64_t* arg_out, void* slab, size_t slab_bytes, int32_t stages, void* stream) {
  MP_DEVICE_GUARD(stream);
  int rc = check_graph(g, "mp_aggregate_f32");
  if (rc) return rc;
  MP_CHECK_ARG(F > 0, "mp_aggregate_f32: F must be positive");
  MP_CHECK_ARG(out != nullptr && (g->n_edges == 0 || x != nullptr), "mp_aggregate_f32: null x/out");
  MP_CHECK_ARG(ldx >= F && ldo >= F, "mp_aggregate_f32: leading dimension < F");
  const bool is_arg = reduce == MP_REDUCE_MAX || reduce == MP_REDUCE_MIN;
  MP_CHECK_ARG(!is_arg || arg_out != nullptr, "mp_aggregate_f32: max/min need arg_out");
  MP_CHECK_ARG(slab != nullptr && slab_bytes >= mp_aggregate_slab_bytes(g, F, reduce),
               "mp_aggregate_f32: slab workspace too small (%zu < %zu)", slab_bytes,
               mp_aggregate_slab_bytes(g, F, reduce));
  MP_CHECK_ARG(reduce >= MP_REDUCE_SUM && reduce <= MP_REDUCE_MIN, "mp_aggregate_f32: unknown reduce %d", reduce);
  AggArgs a{};
  fill_graph(a, g);
  a.F = F;
  a.w = w;
  a.x = x;
  a.ldx = ldx;
  a.flags = flags;
  a.bias = bias;
  a.out = out;
  a.ldo = ldo;
  a.arg_out = arg_out;
  carve_slabs(a, slab, is_arg ? kSlabArg : 0);
  return run(choose(a, g, reduce), a, stages, as_stream(stream));
}

int mp_aggregate_tiles_f32(const mp_csr* g, const float* w, const float* x, int64_t ldx, int32_t x_tile_w,
                           int64_t x_tile_stride, int32_t F, int32_t reduce, int32_t flags, const float* bias,
                           const int32_t* bias_rows, float* out, int64_t ldo, int32_t out_tile_w,
                           int64_t out_tile_stride, void* slab, size_t slab_bytes, int32_t stages, void* stream) {
  MP_DEVICE_GUARD(stream);
  int rc = check_graph(g, "mp_aggregate_tiles_f32");
  if (rc) return rc;
  MP_CHECK_ARG(reduce == MP_REDUCE_SUM || reduce == MP_REDUCE_MEAN, "mp_aggregate_tiles_f32: sum or mean only");
  MP_CHECK_ARG(F > 0 && F % 64 == 0, "mp_aggregate_tiles_f32: F must be a positive multiple of 64");
  MP_CHECK_ARG((flags & ~(MP_FLAG_INIT_FROM_OUT | MP_FLAG_SKIP_EMPTY)) == 0,
               "mp_aggregate_tiles_f32: flags may only hold INIT_FROM_OUT and SKIP_EMPTY");
  MP_CHECK_ARG(!(bias_rows && bias && (flags & MP_FLAG_SKIP_EMPTY)),
               "mp_aggregate_tiles_f32: per-row bias flags and SKIP_EMPTY are separate calls (one kernel each)");
  MP_CHECK_ARG(out != nullptr && (g->n_edges == 0 || (x != nullptr && g->col != nullptr && g->n_cols > 0)),
               "mp_aggregate_tiles_f32: null x/out or a graph without columns");
  MP_CHECK_ARG(x_tile_w >= 0 && out_tile_w >= 0, "mp_aggregate_tiles_f32: negative tile width");
  const int64_t ncols = g->n_cols > 0 ? g->n_cols : 0;
  if (x_tile_w) {
    MP_CHECK_ARG(x_tile_w % 64 == 0 && F % x_tile_w == 0 && x_tile_stride >= ncols * x_tile_w,
                 "mp_aggregate_tiles_f32: x tiles must be 64k features wide, divide F, and not overlap "
                 "(stride %lld < %lld rows x %d)", (long long)x_tile_stride, (long long)ncols, (int)x_tile_w);
  } else {
    MP_CHECK_ARG(ldx >= F, "mp_aggregate_tiles_f32: ldx < F");
  }
  MP_CHECK_ARG(ncols * (x_tile_w ? x_tile_w : ldx) * 4 <= 0xFFFFFFF0LL,
               "mp_aggregate_tiles_f32: one x tile must span < 4 GiB");
  if (out_tile_w) {
    MP_CHECK_ARG(out_tile_w % 64 == 0 && F % out_tile_w == 0 && out_tile_stride >= g->n_rows * out_tile_w,
                 "mp_aggregate_tiles_f32: out tiles must be 64k features wide, divide F, and not overlap "
                 "(stride %lld < %lld rows x %d)", (long long)out_tile_stride, (long long)g->n_rows,
                 (int)out_tile_w);
  } else {
    MP_CHECK_ARG(ldo >= F, "mp_aggregate_tiles_f32: ldo < F");
  }
  MP_CHECK_ARG(slab != nullptr && slab_bytes >= mp_aggregate_slab_bytes(g, F, reduce),
               "mp_aggregate_tiles_f32: slab workspace too small (%zu < %zu)", slab_bytes,
               mp_aggregate_slab_bytes(g, F, reduce));
  AggArgs a{};
  fill_graph(a, g);
  a.F = F;
  a.w = w;
  a.x = x;
  a.ldx = x_tile_w ? x_tile_w : ldx;
  a.x_tw = x_tile_w;
  a.x_ts = x_tile_stride;
  a.flags = flags;
  a.bias = bias;
  a.bias_rows = bias ? bias_rows : nullptr;  // the flags matter only with a bias
  a.out = out;
  a.ldo = out_tile_w ? out_tile_w : ldo;
  a.o_tw = out_tile_w;
  a.o_ts = out_tile_stride;
  carve_slabs(a, slab, 0);
  // every call takes the scalar-batch flat kernel with 64-feature tiles (its
  // instance chosen by the operands' layout and the call's options), row-major
  // operands included: the same kernel mp_aggregate_f32 picks for such rows,
  // with the feature-tile order chosen for the pass's x (see choose)
  return run(choose(a, g, reduce, true), a, stages, as_stream(stream));
}

int mp_aggregate_kernel_name(const mp_csr* g, const float* w, const float* x, int64_t ldx, int32_t F,
                             int32_t reduce, const float* bias, const float* out, int64_t ldo, char* buf,
                             size_t buf_len, void* stream) {
  int rc = check_graph(g, "mp_aggregate_kernel_name");
  if (rc) return rc;
  MP_CHECK_ARG(F > 0 && ldx >= F && ldo >= F && buf != nullptr && buf_len > 0,
               "mp_aggregate_kernel_name: bad arguments");
  MP_CHECK_ARG(reduce >= MP_REDUCE_SUM && reduce <= MP_REDUCE_MIN, "mp_aggregate_kernel_name: unknown reduce %d",
               reduce);
  AggArgs a{};
  fill_graph(a, g);
  a.F = F;
  a.w = w;
  a.x = x;
  a.ldx = ldx;
  a.bias = bias;
  a.out = const_cast<float*>(out);
  a.ldo = ldo;
  const char* mangled = hipKernelNameRefByPtr(reinterpret_cast<const void*>(choose(a, g, reduce).main),
                                             as_stream(stream));
  MP_CHECK_ARG(mangled != nullptr, "mp_aggregate_kernel_name: HIP has no name for the kernel (no device?)");
  int st = 0;
  char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
  const char* name = (st == 0 && dem) ? dem : mangled;
  snprintf(buf, buf_len, "%s", name);
  free(dem);
  return MP_OK;
}

int mp_aggregate_heads_f32(const mp_csr* g, const float* w, int32_t H, const float* x, int64_t ldx, int32_t F,
                           float* out, int64_t ldo, void* slab, size_t slab_bytes, int32_t stages, void* stream) {
  MP_DEVICE_GUARD(stream);
  int rc = check_graph(g, "mp_aggregate_heads_f32");
  if (rc) return rc;
  MP_CHECK_ARG(F > 0 && H > 0 && F % H == 0, "mp_aggregate_heads_f32: F must be a positive multiple of H");
  MP_CHECK_ARG(out && (g->n_edges == 0 || (x && w)), "mp_aggregate_heads_f32: null pointer");
  MP_CHECK_ARG(ldx >= F && ldo >= F, "mp_aggregate_heads_f32: leading dimension < F");
  MP_CHECK_ARG(slab && slab_bytes >= mp_aggregate_slab_bytes(g, F, MP_REDUCE_SUM),
               "mp_aggregate_heads_f32: slab workspace too small");
  AggArgs a{};
  fill_graph(a, g);
  a.F = F;
  a.w = w;
  a.x = x;
  a.ldx = ldx;
  a.out = out;
  a.ldo = ldo;
  a.H = H;
  a.C = F / H;
  carve_slabs(a, slab, 0);
  hipStream_t s = as_stream(stream);
  Shape sh = pick_shape(F, ldx, x, ldo, out);
  int vec = sh.vec;
  while (vec > 1 && a.C % vec != 0) vec >>= 1;  // a lane's features must share a head
  if (vec == 4) return launch<HeadSumRed<4>, 4>(a, stages, s, sh.lanes);
  if (vec == 2) return launch<HeadSumRed<2>, 2>(a, stages, s, 64);
  return launch<HeadSumRed<1>, 1>(a, stages, s, 64);
}

int mp_gat_two_pass_ok(int32_t H, int32_t C) {
  return H >= 1 && H <= 16 && (C == 16 || C == 32 || (C >= 64 && C % 64 == 0)) ? 1 : 0;
}

// Two-pass GAT: row statistics (two lane-task passes over a_src), then the
// reference-order weighted aggregation (k_agg_flat<.., GA>, 64-feature tiles).
int mp_gat_softmax_aggregate_f32(const mp_csr* g, const int32_t* slot_row, const float* xw, const float* a_src,
                                 const float* a_dst, int32_t H, int32_t C, float slope, const float* bias,
                                 float* out, int64_t ldo, float* row_stats, void* slab, size_t slab_bytes,
                                 int32_t stages, void* stream) {
  MP_DEVICE_GUARD(stream);
  int rc = check_graph(g, "mp_gat_softmax_aggregate_f32");
  if (rc) return rc;
  MP_CHECK_ARG(mp_gat_two_pass_ok(H, C),
               "mp_gat_softmax_aggregate_f32: needs H <= 16 and C in {16, 32} or a multiple of 64");
  MP_CHECK_ARG(g->n_edges == 0 || g->col != nullptr, "mp_gat_softmax_aggregate_f32: graph needs a column array");
  MP_CHECK_ARG(xw && a_src && a_dst && out && row_stats && (g->n_edges == 0 || slot_row),
               "mp_gat_softmax_aggregate_f32: null input");
  MP_CHECK_ARG((uintptr_t)row_stats % 8 == 0, "mp_gat_softmax_aggregate_f32: row_stats must be 8-byte aligned");
  const int F = H * C;
  MP_CHECK_ARG(ldo >= F, "mp_gat_softmax_aggregate_f32: ldo < H*C");
  MP_CHECK_ARG(slab != nullptr && slab_bytes >= mp_gat_slab_bytes(g, H, C),
               "mp_gat_softmax_aggregate_f32: slab workspace too small");
  hipStream_t s = as_stream(stream);
  AggArgs a{};
  fill_graph(a, g);
  a.a_src = a_src;
  a.a_dst = a_dst;
  a.H = H;
  a.C = C;
  a.slope = slope;
  a.row_stats = row_stats;
  a.slot_row = slot_row;
  a.slab_v = (float*)slab;
  if (stages & MP_STAGE_STATS) {
    // passes 1 and 2: x = a_src [N, H], F = H
    AggArgs t = a;
    t.F = H;
    t.x = a_src;
    t.ldx = H;
    t.slab_ld = slab_ld_for(H);
    rc = run(gat_stats_launch<GatMaxRed<1>>(t), t, MP_STAGE_ALL, s);
    if (rc) return rc;
    rc = run(gat_stats_launch<GatDenRed<1>>(t), t, MP_STAGE_ALL, s);
    if (rc) return rc;
  }
  a.F = F;
  a.w = a_src;  // any non-null pointer: the HAS_W reducer multiplies by the window's alpha
  a.x = xw;
  a.ldx = F;
  a.bias = bias;
  a.out = out;
  a.ldo = ldo;
  a.slab_ld = slab_ld_for(F);
  // the GA instance of k_agg_flat; its fix-up 4 wide when out (and bias) allow
  using Red = SumRed<1, true, false>;
  const AggKernel k = k_agg_flat<Red, 1, kU_Vec1, 64, true>;
  const bool fix4 = F % 4 == 0 && (uintptr_t)out % 16 == 0 && ldo % 4 == 0 && (uintptr_t)bias % 16 == 0;
  return run(fix4 ? with_fixup<SumRed<4, true, false>, 4>(k, main_grid<1, 64>(a), a)
                  : with_fixup<Red, 1>(k, main_grid<1, 64>(a), a),
             a, stages, s);
}

}  // extern "C"
