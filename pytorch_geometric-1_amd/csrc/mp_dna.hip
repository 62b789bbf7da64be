// DNAConv's per-edge attention over layer histories (gfx950).
//
// Per edge e = (j -> i) and head h (a d = C / H wide slice of the channels) the
// layer attends with ONE query, Q_i[h] = lin_q(x_i[T-1])[h], over the T keys and
// values K_j[t][h], V_j[t][h] of the source's history:
//   s_t  = <Q_i[h], K_j[t][h]> / sqrt(d)
//   a_t  = exp(s_t - m) / (sum_u exp(s_u - m) + exp(-m)),  m = max(0, max_t s_t)
//   out_i[h] += norm_e * sum_t keep_t * scale * a_t * V_j[t][h]
// K, V [n, T, C] and Q [n, C] are node-level projections (the caller's GEMMs): no
// [E, T, C] array exists.  The restricted softmax is the ordinary softmax over
// {0, s_1 .. s_T} with the first entry dropped, so the forward is one online
// pass per slot that starts at m = 0, l = 1, acc = 0, and lse = m + log(l) gives
// a_t = exp(s_t - lse) back in the backward.
//
// One lane group owns one (row, head) unit: g = min(64, pow2 >= d) lanes over the
// head's d channels, 64 / g units per wave; a head wider than 64 gives each lane
// DPL = ceil(d / 64) <= 4 channels (c = lane, lane + 64, ...).  A unit visits its
// row's slots in slot order and adds left to right; a dot product is the lanes'
// partial products summed by the DPP butterfly of group_sum.  Every kernel uses
// the same mapping, so a recomputed score has the forward's bits.  fp32,
// deterministic, no atomics.
//
// Rows and tasks.  On a CSR whose merge-path schedule has tasks of at least
// kDnaSplitChunk work units (the layer asks for such a schedule on a graph of
// any size) a unit is (task, head) instead: it walks the task's slots --
// the tail of a row an earlier task began, then the rows it owns -- exactly as
// the engine's k_agg_main does (mp_agg.h), writes a row that ends inside the
// task, and leaves the partial sum of a row cut by a task boundary in a slab
// (slot 2 * task for a continuation, 2 * task + 1 for a head: the engine's sum
// fix-up protocol).  k_dna_fixup then adds a split row's chain of partials in
// task order and writes the row: a hub row of 10^4 slots is walked by 10^2
// tasks at once instead of by one unit.  A row sum is a sum, so the partials
// combine by addition for out, d Q, d K and d V alike.  On smaller schedules
// (tasks of 16 or 32 units: the source backward's slab would be (1 + N / E) / 4
// or / 8 of an [E, T, C] array there) a unit is (row, head) and walks the whole
// row, however long.
//
//   forward       destination CSR; gathers K_j, V_j; writes out [n_rows, C] and,
//                 when asked, lse [n_ids, H] in edge-id order
//   backward dst  destination CSR; d Q_i = sum_e sum_t ds_t K_j[t] / sqrt(d), with
//                 do = norm_e g_i[h], d alpha_t = keep_t scale <do, V_j[t]>,
//                 ds_t = a_t (d alpha_t - sum_u a_u d alpha_u): two sweeps over t
//   backward src  source-keyed CSR; row j stages its own K_j[h], V_j[h] in LDS and
//                 keeps the accumulators d K_j[h], d V_j[h] [T, d] there too (each
//                 lane reads and writes only its own entries: the LDS is a
//                 dynamically indexed register file, no barrier is needed);
//                 gathers Q_i, g_i, norm and lse through the slot's edge id
// Attention dropout: keep_t = drop_hash(seed, (eid * H + h) * T + t) >= threshold,
// threshold and scale as set_drop has them.
#include "mp_agg.h"
#include "mp_workspace.h"

namespace mp {

constexpr int kDnaMaxDpl = 4;                  // channels of one head per lane: d <= 256
constexpr int kDnaMaxTDpl = 48;                // T * DPL: the source backward's LDS, 4 * 256 B * T * DPL <= 48 KiB
constexpr int64_t kDnaMaxRow = 1 << 20;        // floats in one row of K or V (4 MiB)
constexpr int kDnaSplitChunk = 64;             // task size from which the kernels run over tasks: the source backward's
                                               // slab, 4 T C (N + E) / chunk floats, is (1 + N / E) / 16 of an
                                               // [E, T, C] array at 64 and four times that at 16

static inline int dna_dpl(int32_t d) { return (int)ceil_div(d, 64); }

static inline int dna_group_log2(int32_t d) {
  int gl = 0;
  while ((1 << gl) < d && gl < 6) ++gl;
  return gl;
}

struct DnaDrop {
  uint64_t seed;
  uint32_t thr;
  float scale;
  int32_t on;
};

static inline DnaDrop dna_drop(uint64_t seed, float p_drop) {
  DnaDrop dr{seed, 0u, 1.f, 0};
  if (p_drop > 0.f) {
    AggArgs a{};
    set_drop(a, seed, p_drop);
    dr.thr = a.drop_thr;
    dr.scale = a.drop_scale;
    dr.on = 1;
  }
  return dr;
}

// keep_t * scale of entry (id, h, t); 1 without dropout
__device__ __forceinline__ float dna_keep(const DnaDrop& dr, uint64_t base, int t) {
  if (!dr.on) return 1.f;
  return drop_hash(dr.seed, base + (uint64_t)t) >= dr.thr ? dr.scale : 0.f;
}

// the unit (row or task, head) and the channels of one lane
struct DnaUnit {
  int64_t r;
  int h, fl, g;
};
__device__ __forceinline__ bool dna_unit(int64_t n_rows, int32_t H, int32_t glog, int waves, DnaUnit* u) {
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int sub = lane >> glog;
  u->g = 1 << glog;
  u->fl = lane & (u->g - 1);
  const int64_t unit = (((int64_t)blockIdx.x * waves + wave) << (6 - glog)) + sub;
  if (unit >= n_rows * H) return false;
  u->r = unit / H;
  u->h = (int)(unit - u->r * H);
  return true;
}

// The schedule the kernels run over: wave_row == nullptr = one unit per (row, head).
struct DnaSched {
  const int32_t* wave_row;
  const int32_t* wave_slot;
  int32_t n_waves;
};

// body(row, first slot, end slot, slab slot or -1 = the row ends here: write it) for every piece of a
// row the unit `u` (a row, or a task of `sc`) walks, in slot order
template <class Body>
__device__ __forceinline__ void dna_pieces(const DnaSched& sc, const int32_t* __restrict__ rowptr, int64_t u,
                                           Body&& body) {
  if (!sc.wave_row) {
    body(u, rowptr[u], rowptr[u + 1], (int64_t)-1);
    return;
  }
  const int r_first = sc.wave_row[u], r_last = sc.wave_row[u + 1];
  const int e_begin = sc.wave_slot[u], e_end = sc.wave_slot[u + 1];
  const int ce = rowptr[r_first];  // rowptr[n_rows] = n_edges when the task owns no row
  if (e_begin < ce) body((int64_t)r_first - 1, e_begin, ce < e_end ? ce : e_end, 2 * u);
  for (int r = r_first; r < r_last; ++r) {
    const int rs = rowptr[r], re = rowptr[r + 1];
    if (re <= e_end) body((int64_t)r, rs, re, (int64_t)-1);
    else body((int64_t)r, rs, e_end, 2 * u + 1);
  }
}

template <int DPL>
__device__ __forceinline__ void dna_load(const float* __restrict__ p, int fl, int d, float* v) {
#pragma unroll
  for (int u = 0; u < DPL; ++u) v[u] = fl + u * 64 < d ? p[fl + u * 64] : 0.f;
}

template <int DPL>
__device__ __forceinline__ float dna_dot(const float* a, const float* b, int g) {
  float p = 0.f;
#pragma unroll
  for (int u = 0; u < DPL; ++u) p = __fadd_rn(p, __fmul_rn(a[u], b[u]));
  return group_sum(p, g);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int DPL>
__global__ __launch_bounds__(256) void k_dna_fwd(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                 const int32_t* __restrict__ eid, int64_t n_units, DnaSched sc,
                                                 const float* __restrict__ Q, int64_t ldq,
                                                 const float* __restrict__ K, int64_t ldk,
                                                 const float* __restrict__ V, int64_t ldv,
                                                 const float* __restrict__ norm, int32_t T, int32_t H, int32_t d,
                                                 int32_t glog, float rs, DnaDrop dr, float* __restrict__ out,
                                                 int64_t ldo, float* __restrict__ lse, float* __restrict__ slab) {
  DnaUnit un;
  if (!dna_unit(n_units, H, glog, 4, &un)) return;
  const int C = H * d;
  const int hoff = un.h * d;
  dna_pieces(sc, rowptr, un.r, [&](int64_t r, int b, int e, int64_t slot) {
    float q[DPL], o[DPL];
    dna_load<DPL>(Q + r * ldq + hoff, un.fl, d, q);
#pragma unroll
    for (int u = 0; u < DPL; ++u) o[u] = 0.f;
    int32_t nc = 0, ne = 0;
    if (b < e) {
      nc = col[b];
      ne = eid[b];
    }
    for (int s = b; s < e; ++s) {
      const int32_t j = nc;
      const int64_t id = ne;
      if (s + 1 < e) {
        nc = col[s + 1];
        ne = eid[s + 1];
      }
      const float nr = norm ? norm[id] : 1.f;
      const float* kr = K + (int64_t)j * ldk + hoff;
      const float* vr = V + (int64_t)j * ldv + hoff;
      const uint64_t base = ((uint64_t)id * (uint64_t)H + (uint64_t)un.h) * (uint64_t)T;
      float m = 0.f, l = 1.f, acc[DPL];
#pragma unroll
      for (int u = 0; u < DPL; ++u) acc[u] = 0.f;
      for (int t = 0; t < T; ++t) {
        float kv[DPL], vv[DPL];
        dna_load<DPL>(kr + (int64_t)t * C, un.fl, d, kv);
        dna_load<DPL>(vr + (int64_t)t * C, un.fl, d, vv);
        const float sc_t = __fmul_rn(dna_dot<DPL>(q, kv, un.g), rs);
        const float mn = fmaxf(m, sc_t);
        const float cf = expf(m - mn);
        const float ex = expf(sc_t - mn);
        l = __fadd_rn(__fmul_rn(l, cf), ex);
        const float ea = __fmul_rn(ex, dna_keep(dr, base, t));
#pragma unroll
        for (int u = 0; u < DPL; ++u) acc[u] = __fadd_rn(__fmul_rn(acc[u], cf), __fmul_rn(ea, vv[u]));
        m = mn;
      }
      const float inv = 1.f / l;
#pragma unroll
      for (int u = 0; u < DPL; ++u) o[u] = __fadd_rn(o[u], __fmul_rn(nr, __fmul_rn(acc[u], inv)));
      if (lse && un.fl == 0) lse[id * H + un.h] = m + logf(l);
    }
    float* dst = slot < 0 ? out + r * ldo + hoff : slab + slot * C + hoff;
#pragma unroll
    for (int u = 0; u < DPL; ++u) {
      if (un.fl + u * 64 < d) dst[un.fl + u * 64] = o[u];
    }
  });
}

// ---------------------------------------------------------------------------
// backward over the destination CSR: d Q
// ---------------------------------------------------------------------------
template <int DPL>
__global__ __launch_bounds__(256) void k_dna_bwd_dst(const int32_t* __restrict__ rowptr,
                                                     const int32_t* __restrict__ col,
                                                     const int32_t* __restrict__ eid, int64_t n_units, DnaSched sc,
                                                     const float* __restrict__ Q, int64_t ldq,
                                                     const float* __restrict__ K, int64_t ldk,
                                                     const float* __restrict__ V, int64_t ldv,
                                                     const float* __restrict__ norm, const float* __restrict__ G,
                                                     int64_t ldg, const float* __restrict__ lse, int32_t T, int32_t H,
                                                     int32_t d, int32_t glog, float rs, DnaDrop dr,
                                                     float* __restrict__ dQ, int64_t lddq, float* __restrict__ slab) {
  DnaUnit un;
  if (!dna_unit(n_units, H, glog, 4, &un)) return;
  const int C = H * d;
  const int hoff = un.h * d;
  dna_pieces(sc, rowptr, un.r, [&](int64_t r, int b, int e, int64_t slot) {
    float q[DPL], gi[DPL], dq[DPL];
    dna_load<DPL>(Q + r * ldq + hoff, un.fl, d, q);
    dna_load<DPL>(G + r * ldg + hoff, un.fl, d, gi);
#pragma unroll
    for (int u = 0; u < DPL; ++u) dq[u] = 0.f;
    for (int s = b; s < e; ++s) {
      const int32_t j = col[s];
      const int64_t id = eid[s];
      const float nr = norm ? norm[id] : 1.f;
      const float L = lse[id * H + un.h];
      const float* kr = K + (int64_t)j * ldk + hoff;
      const float* vr = V + (int64_t)j * ldv + hoff;
      const uint64_t base = ((uint64_t)id * (uint64_t)H + (uint64_t)un.h) * (uint64_t)T;
      float dout[DPL];
#pragma unroll
      for (int u = 0; u < DPL; ++u) dout[u] = __fmul_rn(nr, gi[u]);
      float S = 0.f;  // sum_u a_u d alpha_u
      for (int t = 0; t < T; ++t) {
        float kv[DPL], vv[DPL];
        dna_load<DPL>(kr + (int64_t)t * C, un.fl, d, kv);
        dna_load<DPL>(vr + (int64_t)t * C, un.fl, d, vv);
        const float a = expf(__fmul_rn(dna_dot<DPL>(q, kv, un.g), rs) - L);
        const float da = __fmul_rn(dna_keep(dr, base, t), dna_dot<DPL>(dout, vv, un.g));
        S = __fadd_rn(S, __fmul_rn(a, da));
      }
      for (int t = 0; t < T; ++t) {
        float kv[DPL], vv[DPL];
        dna_load<DPL>(kr + (int64_t)t * C, un.fl, d, kv);
        dna_load<DPL>(vr + (int64_t)t * C, un.fl, d, vv);
        const float a = expf(__fmul_rn(dna_dot<DPL>(q, kv, un.g), rs) - L);
        const float da = __fmul_rn(dna_keep(dr, base, t), dna_dot<DPL>(dout, vv, un.g));
        const float ds = __fmul_rn(__fmul_rn(a, da - S), rs);
#pragma unroll
        for (int u = 0; u < DPL; ++u) dq[u] = __fadd_rn(dq[u], __fmul_rn(ds, kv[u]));
      }
    }
    float* dst = slot < 0 ? dQ + r * lddq + hoff : slab + slot * C + hoff;
#pragma unroll
    for (int u = 0; u < DPL; ++u) {
      if (un.fl + u * 64 < d) dst[un.fl + u * 64] = dq[u];
    }
  });
}

// ---------------------------------------------------------------------------
// backward over the source-keyed CSR: d K, d V
// ---------------------------------------------------------------------------
// One wave per block.  LDS: four arrays [T * DPL][64], entry (t, u) of lane `lane`
// at (t * DPL + u) * 64 + lane (consecutive lanes in consecutive banks): the row's
// K_j[h], V_j[h] and the accumulators d K_j[h], d V_j[h].  A lane touches only its
// own entries.  A slab slot holds d K | d V, 2 * T * C floats.
template <int DPL>
__global__ __launch_bounds__(64) void k_dna_bwd_src(const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ col,
                                                    const int32_t* __restrict__ eid, int64_t n_units, DnaSched sc,
                                                    const float* __restrict__ Q, int64_t ldq,
                                                    const float* __restrict__ K, int64_t ldk,
                                                    const float* __restrict__ V, int64_t ldv,
                                                    const float* __restrict__ norm, const float* __restrict__ G,
                                                    int64_t ldg, const float* __restrict__ lse, int32_t T, int32_t H,
                                                    int32_t d, int32_t glog, float rs, DnaDrop dr,
                                                    float* __restrict__ dK, int64_t lddk, float* __restrict__ dV,
                                                    int64_t lddv, float* __restrict__ slab) {
  extern __shared__ float dna_lds[];
  DnaUnit un;
  if (!dna_unit(n_units, H, glog, 1, &un)) return;
  const int C = H * d;
  const int hoff = un.h * d;
  const int lane = lane_id();
  const int TD = T * DPL;
  float* Ks = dna_lds + lane;
  float* Vs = Ks + (int64_t)TD * 64;
  float* dKs = Vs + (int64_t)TD * 64;
  float* dVs = dKs + (int64_t)TD * 64;
  dna_pieces(sc, rowptr, un.r, [&](int64_t r, int b, int e, int64_t slot) {
    {
      const float* kr = K + r * ldk + hoff;
      const float* vr = V + r * ldv + hoff;
      for (int t = 0; t < T; ++t) {
        float kv[DPL], vv[DPL];
        dna_load<DPL>(kr + (int64_t)t * C, un.fl, d, kv);
        dna_load<DPL>(vr + (int64_t)t * C, un.fl, d, vv);
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
          const int at = (t * DPL + u) * 64;
          Ks[at] = kv[u];
          Vs[at] = vv[u];
          dKs[at] = 0.f;
          dVs[at] = 0.f;
        }
      }
    }
    for (int s = b; s < e; ++s) {
      const int32_t i = col[s];
      const int64_t id = eid[s];
      const float nr = norm ? norm[id] : 1.f;
      const float L = lse[id * H + un.h];
      const uint64_t base = ((uint64_t)id * (uint64_t)H + (uint64_t)un.h) * (uint64_t)T;
      float q[DPL], dout[DPL];
      dna_load<DPL>(Q + (int64_t)i * ldq + hoff, un.fl, d, q);
      dna_load<DPL>(G + (int64_t)i * ldg + hoff, un.fl, d, dout);
#pragma unroll
      for (int u = 0; u < DPL; ++u) dout[u] = __fmul_rn(nr, dout[u]);
      float S = 0.f;
      for (int t = 0; t < T; ++t) {
        float kv[DPL], vv[DPL];
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
          kv[u] = Ks[(t * DPL + u) * 64];
          vv[u] = Vs[(t * DPL + u) * 64];
        }
        const float a = expf(__fmul_rn(dna_dot<DPL>(q, kv, un.g), rs) - L);
        const float ks = dna_keep(dr, base, t);
        const float da = __fmul_rn(ks, dna_dot<DPL>(dout, vv, un.g));
        S = __fadd_rn(S, __fmul_rn(a, da));
        const float ad = __fmul_rn(a, ks);  // a_t after dropout
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
          const int at = (t * DPL + u) * 64;
          dVs[at] = __fadd_rn(dVs[at], __fmul_rn(ad, dout[u]));
        }
      }
      for (int t = 0; t < T; ++t) {
        float kv[DPL], vv[DPL];
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
          kv[u] = Ks[(t * DPL + u) * 64];
          vv[u] = Vs[(t * DPL + u) * 64];
        }
        const float a = expf(__fmul_rn(dna_dot<DPL>(q, kv, un.g), rs) - L);
        const float da = __fmul_rn(dna_keep(dr, base, t), dna_dot<DPL>(dout, vv, un.g));
        const float ds = __fmul_rn(__fmul_rn(a, da - S), rs);
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
          const int at = (t * DPL + u) * 64;
          dKs[at] = __fadd_rn(dKs[at], __fmul_rn(ds, q[u]));
        }
      }
    }
    const int64_t TC = (int64_t)T * C;
    float* dkr = slot < 0 ? dK + r * lddk + hoff : slab + slot * 2 * TC + hoff;
    float* dvr = slot < 0 ? dV + r * lddv + hoff : slab + slot * 2 * TC + TC + hoff;
    for (int t = 0; t < T; ++t) {
#pragma unroll
      for (int u = 0; u < DPL; ++u) {
        const int c = un.fl + u * 64;
        if (c < d) {
          dkr[(int64_t)t * C + c] = dKs[(t * DPL + u) * 64];
          dvr[(int64_t)t * C + c] = dVs[(t * DPL + u) * 64];
        }
      }
    }
  });
}

// One block column per split row i: out[r, c] = the row's partials slab[slot, off + c] added in task order
// (the head partial of the owning task, then the continuation of every later task up to split_waves[i]).
__global__ __launch_bounds__(256) void k_dna_fixup(const int32_t* __restrict__ wave_row,
                                                   const int32_t* __restrict__ split_waves, int32_t n_waves,
                                                   const float* __restrict__ slab, int64_t slot_floats, int64_t off,
                                                   int64_t width, float* __restrict__ out, int64_t ldo) {
  const int64_t c = (int64_t)blockIdx.y * 256 + threadIdx.x;
  if (c >= width) return;
  const int last = split_waves[blockIdx.x];
  const int r = wave_row[last] - 1;
  int lo = 0, hi = n_waves;  // owner = the last task whose first owned row is <= r (wave_row[n_waves] = n_rows > r)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (wave_row[mid] <= r) lo = mid;
    else hi = mid - 1;
  }
  const int owner = lo;
  const float* p = slab + off + c;
  float t = p[(2 * (int64_t)owner + 1) * slot_floats];
  for (int k = owner + 1; k <= last; ++k) t = __fadd_rn(t, p[2 * (int64_t)k * slot_floats]);
  out[(int64_t)r * ldo + c] = t;
}

// keep[(id * H + h) * T + t] for every id < n_edges, in edge-id order
__global__ __launch_bounds__(256) void k_dna_keep(DnaDrop dr, int64_t n, uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keep[i] = drop_hash(dr.seed, (uint64_t)i) >= dr.thr ? 1 : 0;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int dna_shape(const char* fn, int32_t T, int32_t H, int32_t C) {
  MP_CHECK_ARG(T >= 1, "%s: T = %d < 1", fn, T);
  MP_CHECK_ARG(H >= 1, "%s: H = %d < 1", fn, H);
  MP_CHECK_ARG(C >= 1, "%s: C = %d < 1", fn, C);
  MP_CHECK_ARG(C % H == 0, "%s: C = %d is no multiple of H = %d", fn, C, H);
  const int32_t d = C / H;
  MP_CHECK_ARG(d <= 64 * kDnaMaxDpl, "%s: C / H = %d above the limit C / H <= %d", fn, d, 64 * kDnaMaxDpl);
  MP_CHECK_ARG((int64_t)T * dna_dpl(d) <= kDnaMaxTDpl,
               "%s: T = %d above the limit T * ceil((C / H) / 64) <= %d (C / H = %d)", fn, T, kDnaMaxTDpl, d);
  MP_CHECK_ARG((int64_t)T * C <= kDnaMaxRow, "%s: T * C = %lld above the limit T * C <= %lld", fn,
               (long long)((int64_t)T * C), (long long)kDnaMaxRow);
  return MP_OK;
}

// whether the kernels run over the tasks of g's schedule (else over its rows)
static inline bool dna_tasks(const mp_csr* g) { return g->wave_row != nullptr && g->chunk >= kDnaSplitChunk; }

// The slab of one call: two slots per task (continuation, head) of `slot_floats` floats -- C for the forward
// and d Q, 2 * T * C (d K | d V) for the source backward; nothing for a CSR the kernels walk by rows.
struct DnaWs : Carver {
  float* slab;
  DnaWs(void* ws, int64_t n_waves, int64_t slot_floats) : Carver(ws), slab(take<float>(2 * n_waves * slot_floats)) {}
};

static int dna_csr(const char* fn, const mp_csr* g, const float* norm, int64_t n_norm, const float* lse,
                   size_t lse_bytes, bool lse_required, int32_t H) {
  MP_CHECK_ARG(g != nullptr, "%s: g is NULL", fn);
  MP_CHECK_ARG(g->n_rows >= 0 && g->n_edges >= 0, "%s: negative n_rows / n_edges", fn);
  MP_CHECK_ARG(g->n_rows <= 0x7fffffff && g->n_edges <= 0x7fffffff, "%s: n_rows / n_edges above 2^31 - 1", fn);
  MP_CHECK_ARG(g->rowptr != nullptr, "%s: g->rowptr is NULL", fn);
  MP_CHECK_ARG(g->col != nullptr, "%s: g->col is NULL (the DNA passes gather by column)", fn);
  MP_CHECK_ARG(g->eid != nullptr, "%s: g->eid is NULL (norm and lse are read in original edge order)", fn);
  MP_CHECK_ARG(g->n_cols > 0, "%s: g->n_cols must be > 0", fn);
  if (dna_tasks(g)) {
    MP_CHECK_ARG(g->wave_slot != nullptr, "%s: g->wave_slot is NULL (a schedule with chunk = %d)", fn, g->chunk);
    MP_CHECK_ARG(g->n_waves >= 1, "%s: g->n_waves = %d < 1", fn, g->n_waves);
    MP_CHECK_ARG(g->n_split >= 0 && g->n_split <= g->n_waves, "%s: g->n_split = %d outside [0, n_waves = %d]", fn,
                 g->n_split, g->n_waves);
    MP_CHECK_ARG(g->n_split == 0 || g->split_waves != nullptr, "%s: g->split_waves is NULL with n_split = %d", fn,
                 g->n_split);
  }
  const int64_t ids = g->n_ids > 0 ? g->n_ids : g->n_edges;
  MP_CHECK_ARG(norm == nullptr || n_norm >= ids, "%s: eid indexes %lld edges, norm holds n_norm = %lld", fn,
               (long long)ids, (long long)n_norm);
  MP_CHECK_ARG(!lse_required || lse != nullptr, "%s: lse is NULL", fn);
  if (lse != nullptr) MP_CHECK_EXTENT(fn, "lse", lse_bytes, (size_t)ids * H * sizeof(float));
  return MP_OK;
}

// the slab of a task-walking call, checked; *slab stays NULL for a row-walking one
static int dna_ws(const char* fn, const mp_csr* g, int64_t slot_floats, void* ws, size_t ws_bytes, float** slab) {
  *slab = nullptr;
  if (!dna_tasks(g) || g->n_rows == 0) return MP_OK;
  MP_CHECK_ARG(ws != nullptr, "%s: ws is NULL", fn);
  DnaWs w(ws, g->n_waves, slot_floats);
  MP_CHECK_EXTENT(fn, "ws", ws_bytes, w.total(0));
  *slab = w.slab;
  return MP_OK;
}

// one operand [n, T, C] (or [n, C] with T = 1) under its row stride
static int dna_rows(const char* fn, const char* name, const void* p, int64_t ld, size_t bytes, int64_t n, int64_t row) {
  MP_CHECK_ARG(p != nullptr, "%s: %s is NULL", fn, name);
  MP_CHECK_ARG(ld >= row, "%s: ld of %s = %lld < %lld", fn, name, (long long)ld, (long long)row);
  MP_CHECK_EXTENT(fn, name, bytes, n <= 0 ? 0 : ((size_t)(n - 1) * ld + row) * sizeof(float));
  return MP_OK;
}

static int dna_p(const char* fn, float p_drop) {
  MP_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f, "%s: dropout p must be in [0, 1) (got %g)", fn, (double)p_drop);
  return MP_OK;
}

#define DNA_BY_DPL(kern, dpl) \
  ((dpl) == 1 ? kern<1> : ((dpl) == 2 ? kern<2> : ((dpl) == 3 ? kern<3> : kern<4>)))

// what every launch of one call shares
struct DnaLaunch {
  DnaSched sc;
  int64_t n_units, blocks;
  int32_t d, glog, dpl;
  float rs;
};
static int dna_launch(const char* fn, const mp_csr* g, int32_t H, int32_t C, int waves, DnaLaunch* l) {
  l->sc = dna_tasks(g) ? DnaSched{g->wave_row, g->wave_slot, g->n_waves} : DnaSched{nullptr, nullptr, 0};
  l->n_units = dna_tasks(g) ? (int64_t)g->n_waves : g->n_rows;
  l->d = C / H;
  l->glog = dna_group_log2(l->d);
  l->dpl = dna_dpl(l->d);
  l->rs = (float)(1.0 / std::sqrt((double)l->d));
  l->blocks = ceil_div(l->n_units * H, (int64_t)waves << (6 - l->glog));
  MP_CHECK_ARG(l->blocks <= 0x7fffffff, "%s: grid too large (%lld rows or tasks, H %d)", fn, (long long)l->n_units, H);
  return MP_OK;
}

// the fix-up of one output [n_rows, width] whose partials sit at `off` of every slab slot
static int dna_fixup(const mp_csr* g, const float* slab, int64_t slot_floats, int64_t off, int64_t width, float* out,
                     int64_t ldo, void* stream, int64_t* launches) {
  if (slab == nullptr || g->n_split == 0) return MP_OK;
  hipLaunchKernelGGL(k_dna_fixup, dim3((unsigned)g->n_split, (unsigned)ceil_div(width, 256)), dim3(256), 0,
                     as_stream(stream), g->wave_row, g->split_waves, g->n_waves, slab, slot_floats, off, width, out, ldo);
  MP_CHECK_LAUNCH();
  ++*launches;
  return MP_OK;
}

static int dna_aggregate(const mp_csr* g, const float* q, int64_t ldq, size_t q_bytes, const float* k, int64_t ldk,
                         size_t k_bytes, const float* v, int64_t ldv, size_t v_bytes, const float* norm,
                         int64_t n_norm, int32_t T, int32_t H, int32_t C, uint64_t seed, float p_drop, float* out,
                         int64_t ldo, size_t out_bytes, float* lse, size_t lse_bytes, void* ws, size_t ws_bytes,
                         void* stream, int64_t* launches) {
  const char* fn = "mp_dna_aggregate_f32";
  if (int rc = dna_shape(fn, T, H, C)) return rc;
  if (int rc = dna_p(fn, p_drop)) return rc;
  if (int rc = dna_csr(fn, g, norm, n_norm, lse, lse_bytes, false, H)) return rc;
  if (int rc = dna_rows(fn, "q", q, ldq, q_bytes, g->n_rows, C)) return rc;
  if (int rc = dna_rows(fn, "k", k, ldk, k_bytes, g->n_cols, (int64_t)T * C)) return rc;
  if (int rc = dna_rows(fn, "v", v, ldv, v_bytes, g->n_cols, (int64_t)T * C)) return rc;
  if (int rc = dna_rows(fn, "out", out, ldo, out_bytes, g->n_rows, C)) return rc;
  float* slab;
  if (int rc = dna_ws(fn, g, C, ws, ws_bytes, &slab)) return rc;
  if (g->n_rows == 0) return MP_OK;
  DnaLaunch l;
  if (int rc = dna_launch(fn, g, H, C, 4, &l)) return rc;
  MP_DEVICE_GUARD(stream);
  hipLaunchKernelGGL(DNA_BY_DPL(k_dna_fwd, l.dpl), dim3((unsigned)l.blocks), dim3(256), 0, as_stream(stream),
                     g->rowptr, g->col, g->eid, l.n_units, l.sc, q, ldq, k, ldk, v, ldv, norm, T, H, l.d, l.glog, l.rs,
                     dna_drop(seed, p_drop), out, ldo, lse, slab);
  MP_CHECK_LAUNCH();
  ++*launches;
  return dna_fixup(g, slab, C, 0, C, out, ldo, stream, launches);
}

static int dna_backward_dst(const mp_csr* g, const float* q, int64_t ldq, size_t q_bytes, const float* k, int64_t ldk,
                            size_t k_bytes, const float* v, int64_t ldv, size_t v_bytes, const float* norm,
                            int64_t n_norm, const float* gout, int64_t ldg, size_t g_bytes, const float* lse,
                            size_t lse_bytes, int32_t T, int32_t H, int32_t C, uint64_t seed, float p_drop, float* dq,
                            int64_t lddq, size_t dq_bytes, void* ws, size_t ws_bytes, void* stream,
                            int64_t* launches) {
  const char* fn = "mp_dna_backward_dst_f32";
  if (int rc = dna_shape(fn, T, H, C)) return rc;
  if (int rc = dna_p(fn, p_drop)) return rc;
  if (int rc = dna_csr(fn, g, norm, n_norm, lse, lse_bytes, g != nullptr && g->n_edges > 0, H)) return rc;
  if (int rc = dna_rows(fn, "q", q, ldq, q_bytes, g->n_rows, C)) return rc;
  if (int rc = dna_rows(fn, "k", k, ldk, k_bytes, g->n_cols, (int64_t)T * C)) return rc;
  if (int rc = dna_rows(fn, "v", v, ldv, v_bytes, g->n_cols, (int64_t)T * C)) return rc;
  if (int rc = dna_rows(fn, "gout", gout, ldg, g_bytes, g->n_rows, C)) return rc;
  if (int rc = dna_rows(fn, "dq", dq, lddq, dq_bytes, g->n_rows, C)) return rc;
  float* slab;
  if (int rc = dna_ws(fn, g, C, ws, ws_bytes, &slab)) return rc;
  if (g->n_rows == 0) return MP_OK;
  DnaLaunch l;
  if (int rc = dna_launch(fn, g, H, C, 4, &l)) return rc;
  MP_DEVICE_GUARD(stream);
  hipLaunchKernelGGL(DNA_BY_DPL(k_dna_bwd_dst, l.dpl), dim3((unsigned)l.blocks), dim3(256), 0, as_stream(stream),
                     g->rowptr, g->col, g->eid, l.n_units, l.sc, q, ldq, k, ldk, v, ldv, norm, gout, ldg, lse, T, H, l.d,
                     l.glog, l.rs, dna_drop(seed, p_drop), dq, lddq, slab);
  MP_CHECK_LAUNCH();
  ++*launches;
  return dna_fixup(g, slab, C, 0, C, dq, lddq, stream, launches);
}

static int dna_backward_src(const mp_csr* g, const float* q, int64_t ldq, size_t q_bytes, const float* k, int64_t ldk,
                            size_t k_bytes, const float* v, int64_t ldv, size_t v_bytes, const float* norm,
                            int64_t n_norm, const float* gout, int64_t ldg, size_t g_bytes, const float* lse,
                            size_t lse_bytes, int32_t T, int32_t H, int32_t C, uint64_t seed, float p_drop, float* dk,
                            int64_t lddk, size_t dk_bytes, float* dv, int64_t lddv, size_t dv_bytes, void* ws,
                            size_t ws_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_dna_backward_src_f32";
  if (int rc = dna_shape(fn, T, H, C)) return rc;
  if (int rc = dna_p(fn, p_drop)) return rc;
  if (int rc = dna_csr(fn, g, norm, n_norm, lse, lse_bytes, g != nullptr && g->n_edges > 0, H)) return rc;
  // rows are the sources (k, v, dk, dv), columns the destinations (q, gout)
  const int64_t TC = (int64_t)T * C;
  if (int rc = dna_rows(fn, "q", q, ldq, q_bytes, g->n_cols, C)) return rc;
  if (int rc = dna_rows(fn, "gout", gout, ldg, g_bytes, g->n_cols, C)) return rc;
  if (int rc = dna_rows(fn, "k", k, ldk, k_bytes, g->n_rows, TC)) return rc;
  if (int rc = dna_rows(fn, "v", v, ldv, v_bytes, g->n_rows, TC)) return rc;
  if (int rc = dna_rows(fn, "dk", dk, lddk, dk_bytes, g->n_rows, TC)) return rc;
  if (int rc = dna_rows(fn, "dv", dv, lddv, dv_bytes, g->n_rows, TC)) return rc;
  float* slab;
  if (int rc = dna_ws(fn, g, 2 * TC, ws, ws_bytes, &slab)) return rc;
  if (g->n_rows == 0) return MP_OK;
  DnaLaunch l;
  if (int rc = dna_launch(fn, g, H, C, 1, &l)) return rc;
  const size_t lds = (size_t)4 * T * l.dpl * 64 * sizeof(float);  // <= 4 * kDnaMaxTDpl * 256 B = 48 KiB (dna_shape)
  MP_DEVICE_GUARD(stream);
  hipLaunchKernelGGL(DNA_BY_DPL(k_dna_bwd_src, l.dpl), dim3((unsigned)l.blocks), dim3(64), lds, as_stream(stream),
                     g->rowptr, g->col, g->eid, l.n_units, l.sc, q, ldq, k, ldk, v, ldv, norm, gout, ldg, lse, T, H, l.d,
                     l.glog, l.rs, dna_drop(seed, p_drop), dk, lddk, dv, lddv, slab);
  MP_CHECK_LAUNCH();
  ++*launches;
  if (int rc = dna_fixup(g, slab, 2 * TC, 0, TC, dk, lddk, stream, launches)) return rc;
  return dna_fixup(g, slab, 2 * TC, TC, TC, dv, lddv, stream, launches);
}

static int dna_keep_mask(uint64_t seed, float p_drop, int32_t H, int32_t T, int64_t n_edges, uint8_t* keep,
                         size_t keep_bytes, void* stream) {
  const char* fn = "mp_dna_dropout_keep";
  MP_CHECK_ARG(p_drop > 0.f && p_drop < 1.f, "%s: dropout p must be in (0, 1) (got %g)", fn, (double)p_drop);
  MP_CHECK_ARG(H >= 1, "%s: H = %d < 1", fn, H);
  MP_CHECK_ARG(T >= 1, "%s: T = %d < 1", fn, T);
  MP_CHECK_ARG(n_edges >= 0, "%s: n_edges < 0", fn);
  MP_CHECK_ARG(n_edges <= ((int64_t)1 << 38) / ((int64_t)H * T), "%s: n_edges * H * T too large", fn);
  const int64_t n = n_edges * H * T;
  MP_CHECK_ARG(keep != nullptr || n == 0, "%s: keep is NULL", fn);
  MP_CHECK_EXTENT(fn, "keep", keep_bytes, (size_t)n);
  if (n == 0) return MP_OK;
  MP_DEVICE_GUARD(stream);
  hipLaunchKernelGGL(k_dna_keep, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, as_stream(stream),
                     dna_drop(seed, p_drop), n, keep);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static inline int64_t dna_result(int rc, int64_t launches) { return rc != MP_OK ? -(int64_t)rc : launches; }

}  // namespace mp

using namespace mp;

extern "C" int64_t mp_dna_ok(int32_t T, int32_t H, int32_t C) { return dna_shape("mp_dna_ok", T, H, C) == MP_OK ? 1 : 0; }

extern "C" int64_t mp_dna_max_layers(int32_t H, int32_t C) {
  if (H < 1 || C < 1 || C % H != 0 || C / H > 64 * kDnaMaxDpl) return 0;
  const int64_t by_lds = kDnaMaxTDpl / dna_dpl(C / H);
  const int64_t by_row = kDnaMaxRow / C;
  return by_lds < by_row ? by_lds : by_row;
}

extern "C" int64_t mp_dna_split_chunk(void) { return kDnaSplitChunk; }

extern "C" size_t mp_dna_workspace(const mp_csr* g, int64_t slot_floats) {
  if (g == nullptr || slot_floats < 1 || !dna_tasks(g) || g->n_waves < 1) return DnaWs{nullptr, 0, 1}.total(0);
  return DnaWs{nullptr, g->n_waves, slot_floats}.total(0);
}

extern "C" int64_t mp_dna_aggregate_f32(const mp_csr* g, const float* q, int64_t ldq, size_t q_bytes, const float* k,
                                        int64_t ldk, size_t k_bytes, const float* v, int64_t ldv, size_t v_bytes,
                                        const float* norm, int64_t n_norm, int32_t T, int32_t H, int32_t C,
                                        uint64_t seed, float p_drop, float* out, int64_t ldo, size_t out_bytes,
                                        float* lse, size_t lse_bytes, void* ws, size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = dna_aggregate(g, q, ldq, q_bytes, k, ldk, k_bytes, v, ldv, v_bytes, norm, n_norm, T, H, C, seed,
                               p_drop, out, ldo, out_bytes, lse, lse_bytes, ws, ws_bytes, stream, &launches);
  return dna_result(rc, launches);
}

extern "C" int64_t mp_dna_backward_dst_f32(const mp_csr* g, const float* q, int64_t ldq, size_t q_bytes,
                                           const float* k, int64_t ldk, size_t k_bytes, const float* v, int64_t ldv,
                                           size_t v_bytes, const float* norm, int64_t n_norm, const float* gout,
                                           int64_t ldg, size_t g_bytes, const float* lse, size_t lse_bytes, int32_t T,
                                           int32_t H, int32_t C, uint64_t seed, float p_drop, float* dq, int64_t lddq,
                                           size_t dq_bytes, void* ws, size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = dna_backward_dst(g, q, ldq, q_bytes, k, ldk, k_bytes, v, ldv, v_bytes, norm, n_norm, gout, ldg,
                                  g_bytes, lse, lse_bytes, T, H, C, seed, p_drop, dq, lddq, dq_bytes, ws, ws_bytes,
                                  stream, &launches);
  return dna_result(rc, launches);
}

extern "C" int64_t mp_dna_backward_src_f32(const mp_csr* g, const float* q, int64_t ldq, size_t q_bytes,
                                           const float* k, int64_t ldk, size_t k_bytes, const float* v, int64_t ldv,
                                           size_t v_bytes, const float* norm, int64_t n_norm, const float* gout,
                                           int64_t ldg, size_t g_bytes, const float* lse, size_t lse_bytes, int32_t T,
                                           int32_t H, int32_t C, uint64_t seed, float p_drop, float* dk, int64_t lddk,
                                           size_t dk_bytes, float* dv, int64_t lddv, size_t dv_bytes, void* ws,
                                           size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = dna_backward_src(g, q, ldq, q_bytes, k, ldk, k_bytes, v, ldv, v_bytes, norm, n_norm, gout, ldg,
                                  g_bytes, lse, lse_bytes, T, H, C, seed, p_drop, dk, lddk, dk_bytes, dv, lddv,
                                  dv_bytes, ws, ws_bytes, stream, &launches);
  return dna_result(rc, launches);
}

extern "C" int64_t mp_dna_dropout_keep(uint64_t seed, float p_drop, int32_t H, int32_t T, int64_t n_edges,
                                       uint8_t* keep, size_t keep_bytes, void* stream) {
  const int rc = dna_keep_mask(seed, p_drop, H, T, n_edges, keep, keep_bytes, stream);
  return dna_result(rc, n_edges > 0 ? 1 : 0);
}
